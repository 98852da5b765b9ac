"""The processed verifying key on the MI355X (see tests/pvk_cases.py): `ark355_pvk_pairings` byte for byte against
`ark355_pairing_groups` across the ends of a wave and a third workgroup, `ark355_verify_each_pvk` against
`ark355_verify_each` with five kinds of tampering, under the default policy and past the chunk, the key shapes, the batch
entry, sharing between contexts and the refusals."""
import pytest

import pairing_cases as P
import pvk_cases as K
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


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_pairings_match_pairing_groups(gpu_lib, gpu_ctx, device_route, C, n):
    K.pairings_match_groups_case(gpu_lib, gpu_ctx, C, n, inf=tuple(i for i in (0, 64) if i < n and n > 1))


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_pairings_routes_agree(gpu_lib, gpu_ctx, gpu_policy, C):
    gpu_policy.setenv("ARK355_PAIRING_DEVICE", 0)
    K.pairings_match_groups_case(gpu_lib, gpu_ctx, C, 5, whiches=(2,), inf=(3,))


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_pairings_against_the_oracle(gpu_lib, gpu_ctx, device_route, C):
    K.pairings_oracle_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_pairings_with_delta_at_infinity(gpu_lib, gpu_ctx, device_route, C):
    K.delta_at_infinity_pairings_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_pvk_alpha_beta(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    K.alpha_beta_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name][0])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_pvk_130(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    K.verify_each_pvk_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_pvk_4096_default_policy(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    K.verify_each_pvk_default_policy_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name])


@pytest.mark.parametrize("total", [10923, 32769])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_pvk_past_the_chunk(gpu_lib, gpu_ctx, device_route, oracle_batches, C, total):
    assert total in (K.each_chunk_proofs() + 1, (1 << 15) // 3 + 1)
    K.past_the_chunk_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name], total)


@pytest.mark.parametrize("delta_inf", [False, True], ids=["delta", "delta-at-infinity"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_pvk_without_public_inputs(gpu_lib, gpu_ctx, device_route, C, delta_inf):
    K.no_public_inputs_case(gpu_lib, gpu_ctx, C, delta_inf=delta_inf)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_gamma_outside_the_subgroup_returns_cleanly(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    K.non_subgroup_gamma_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_pvk(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    K.verify_batch_pvk_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_handle_is_shared_between_contexts_and_outlives_its_own(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    K.sharing_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    K.refusals_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name], Ark355Error, EINVAL)


def test_groth16_process_vk_and_verify_with_processed_vk(gpu_lib, oracle_batches):
    K.groth16_mirror_case(gpu_lib, BLS12_381, oracle_batches["bls12_381"])
