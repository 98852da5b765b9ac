"""Per-group pairings behind the C ABI on the CPU emulator build (see tests/pairing_each_cases.py): the per-pair
accumulation, the final-exponentiation kernel and the kernels of `ark355_verify_each` compiled with g++ against the HIP
emulator, at sizes a single host thread handles."""
import pytest

import pairing_cases as P
import pairing_each_cases as E
from conftest import ROOT
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error


@pytest.fixture
def device_route(emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return emul_policy


@pytest.fixture(scope="module")
def small_batches():
    """3 oracle-made proofs of one key per curve"""
    return {C.name: P.oracle_batch(C, 3) for C in (BLS12_381, BN254)}


@pytest.mark.parametrize("C,groups,group_len", [(BLS12_381, 1, 1), (BLS12_381, 2, 1), (BN254, 2, 2)],
                         ids=["bls-1x1", "bls-2x1", "bn-2x2"])
def test_gt_per_group_against_the_oracle(emul_lib, emul_ctx, device_route, C, groups, group_len):
    E.gt_groups_case(emul_lib, emul_ctx, C, groups, group_len)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_groups_match_multi_pairing(emul_lib, emul_ctx, device_route, C):
    E.groups_match_multi_pairing_case(emul_lib, emul_ctx, C, 1, 2)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_routes_agree(emul_lib, emul_ctx, emul_policy, C):
    E.routes_agree_each_case(emul_lib, emul_ctx, emul_policy, C, 2, 1)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_verify_each(emul_lib, emul_ctx, emul_policy, small_batches, C):
    E.verify_each_case(emul_lib, emul_ctx, emul_policy, C, small_batches[C.name], Ark355Error, EINVAL, total=3,
                       tamper=dict(other_c=(1,)), singles=(0,))


def test_verify_each_without_public_inputs(emul_lib, emul_ctx, device_route):
    E.no_public_inputs_case(emul_lib, emul_ctx, BN254)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_refusals(emul_lib, emul_ctx, device_route, C):
    E.refusals_each_case(emul_lib, emul_ctx, C, Ark355Error, EINVAL)


def test_refusals_on_the_host_route(emul_lib, emul_ctx, emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 0)
    E.refusals_each_case(emul_lib, emul_ctx, BLS12_381, Ark355Error, EINVAL)


def test_default_route(emul_lib):
    E.default_each_route_case(emul_lib, ROOT)
