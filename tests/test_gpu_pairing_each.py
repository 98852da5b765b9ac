"""Per-group pairings on the MI355X (see tests/pairing_each_cases.py): `ark355_pairing_groups` against oracle/pairing.py
group by group, the host route against the device route, a call past the 2^15-pair chunk, and `ark355_verify_each` up to
4096 proofs under the default policy."""
import pytest

import pairing_cases as P
import pairing_each_cases as E
from conftest import ROOT
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error

pytestmark = pytest.mark.gpu

CURVES = [BLS12_381, BN254]


@pytest.fixture
def device_route(gpu_policy):
    gpu_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return gpu_policy


@pytest.fixture(scope="module")
def oracle_batches():
    """8 oracle-made proofs of one key per curve, made once"""
    return {C.name: P.oracle_batch(C, 8) for C in CURVES}


@pytest.mark.parametrize("groups,group_len", E.GT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_gt_per_group_against_the_oracle(gpu_lib, gpu_ctx, device_route, C, groups, group_len):
    E.gt_groups_case(gpu_lib, gpu_ctx, C, groups, group_len)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_groups_match_multi_pairing(gpu_lib, gpu_ctx, device_route, C):
    E.groups_match_multi_pairing_case(gpu_lib, gpu_ctx, C, 5, 3)


@pytest.mark.parametrize("groups,group_len", [(200, 1), (67, 3)], ids=lambda v: str(v))
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_routes_agree(gpu_lib, gpu_ctx, gpu_policy, C, groups, group_len):
    E.routes_agree_each_case(gpu_lib, gpu_ctx, gpu_policy, C, groups, group_len)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_past_the_pair_chunk(gpu_lib, gpu_ctx, device_route, C):
    E.chunk_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(gpu_lib, gpu_ctx, device_route, C):
    E.refusals_each_case(gpu_lib, gpu_ctx, C, Ark355Error, EINVAL, groups=5, group_len=3)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_130(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    E.verify_each_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name], Ark355Error, EINVAL)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_4096_default_policy(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    E.verify_each_default_policy_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_without_public_inputs(gpu_lib, gpu_ctx, device_route, C):
    E.no_public_inputs_case(gpu_lib, gpu_ctx, C)


def test_default_route(gpu_lib):
    E.default_each_route_case(gpu_lib, ROOT)
