"""The processed verifying key behind the C ABI on the CPU emulator build (see tests/pvk_cases.py): the key-lines kernel, the
pass B against prepared points and the drivers of the `*_pvk` entries compiled with g++ against the HIP emulator, at sizes a
single host thread handles."""
import pytest

import pairing_cases as P
import pvk_cases as K
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error

CURVES = [BLS12_381, BN254]


@pytest.fixture
def device_route(emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return emul_policy


@pytest.fixture(scope="module")
def small_batches():
    """3 oracle-made proofs of one key per curve"""
    return {C.name: P.oracle_batch(C, 3) for C in CURVES}


@pytest.mark.parametrize("C,which", [(BLS12_381, 1), (BN254, 2)], ids=["bls-gamma", "bn-delta"])
def test_pvk_pairings_match_pairing_groups(emul_lib, emul_ctx, device_route, C, which):
    K.pairings_match_groups_case(emul_lib, emul_ctx, C, 3, whiches=(which,), inf=(1,))


def test_pvk_pairings_on_the_host_route(emul_lib, emul_ctx, emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 0)
    K.pairings_match_groups_case(emul_lib, emul_ctx, BN254, 2, whiches=(0,), inf=(0,))


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_alpha_beta(emul_lib, emul_ctx, device_route, small_batches, C):
    K.alpha_beta_case(emul_lib, emul_ctx, C, small_batches[C.name][0])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_pvk(emul_lib, emul_ctx, emul_policy, small_batches, C):
    K.verify_each_pvk_case(emul_lib, emul_ctx, emul_policy, C, small_batches[C.name], total=3, tamper=dict(other_c=(1,)))


def test_verify_each_pvk_without_public_inputs(emul_lib, emul_ctx, device_route):
    K.no_public_inputs_case(emul_lib, emul_ctx, BN254)


def test_verify_batch_pvk(emul_lib, emul_ctx, device_route, small_batches):
    K.verify_batch_pvk_case(emul_lib, emul_ctx, BN254, small_batches["bn254"], count=1)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(emul_lib, emul_ctx, device_route, small_batches, C):
    K.refusals_case(emul_lib, emul_ctx, C, small_batches[C.name], Ark355Error, EINVAL)


def test_handle_outlives_its_context(emul_lib, emul_ctx, device_route, small_batches):
    K.sharing_case(emul_lib, emul_ctx, BN254, small_batches["bn254"], total=2)


def test_groth16_process_vk_and_verify_with_processed_vk(emul_lib, small_batches):
    K.groth16_mirror_case(emul_lib, BN254, small_batches["bn254"])
