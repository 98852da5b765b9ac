"""GPU tier of the h query in the evaluation basis (policy H_EVAL; snark_amd/csrc/hbasis_impl.cuh): the cases of
tests/hbasis_cases.py on the device, and what only a device shows -- two contexts meeting a fresh key at once, the default policy
at the smallest domain it converts."""
import pytest

import hbasis_cases as H
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
PATHS = pytest.mark.parametrize("h_eval", [1, 0], ids=["H_EVAL=1", "H_EVAL=0"])


@CURVES
@pytest.mark.parametrize("log_n", [1, 3, 6])
def test_group_transforms_vs_direct_sums(gpu_lib, gpu_ctx, C, log_n):
    H.transform_case(gpu_lib, gpu_ctx, C, log_n)


@CURVES
def test_group_transform_with_infinity_inside(gpu_lib, gpu_ctx, C):
    H.transform_case(gpu_lib, gpu_ctx, C, 3, inf_at=(2, 5))


@CURVES
def test_gather_hand_built_columns(gpu_lib, gpu_ctx, C):
    H.gather_hand_built_case(gpu_lib, gpu_ctx, C)


@CURVES
@pytest.mark.parametrize("n", [(1 << 11) + 1, (1 << 11) + 2], ids=["one-full-chunk", "two-chunks"])
def test_gather_heavy_column(gpu_lib, gpu_ctx, C, n):
    H.gather_heavy_case(gpu_lib, gpu_ctx, C, n)


@CURVES
def test_gather_column_lengths(gpu_lib, gpu_ctx, C):
    """columns of 63, 64, 65, 2048, 2049 and 0 entries: both sides of the lane limit and of the chunk, with scalar multiplications"""
    H.gather_lengths_case(gpu_lib, gpu_ctx, C)


@PATHS
@pytest.mark.parametrize("name", ["mulchain-6", "mulchain-32", "golden", "ell1"])
def test_proofs_match_the_oracle_on_both_paths(gpu_lib, gpu_ctx, gpu_policy, name, h_eval):
    H.prove_rows_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy, name, h_eval)


@PATHS
def test_proofs_bn254(gpu_lib, gpu_ctx, gpu_policy, h_eval):
    H.prove_rows_case(gpu_lib, gpu_ctx, BN254, gpu_policy, "mulchain-6", h_eval)


@PATHS
@pytest.mark.parametrize("name", ["mulchain-1022", "dummy-256"])
def test_proofs_match_oracle_c_on_both_paths(gpu_lib, gpu_ctx, gpu_policy, name, h_eval):
    """mulchain at n = 2^10 - 2: N = 2^10, the smallest domain with the fused inverse -> coset seam; the DummyCircuit at 2^8."""
    H.prove_csr_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy, name, h_eval)


@PATHS
def test_unsatisfied_assignment_proves_like_the_seven_transform_prover(gpu_lib, gpu_ctx, gpu_policy, h_eval):
    H.prove_rows_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy, "mulchain-6", h_eval, unsatisfied=True)


def test_check_satisfied_on_a_bound_key(gpu_lib, gpu_ctx, gpu_policy):
    H.check_satisfied_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy)


def test_bound_key_refuses_another_r1cs_handle(gpu_lib, gpu_ctx, gpu_policy):
    H.other_r1cs_refused_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy)


def test_key_shards_keep_the_coefficient_path(gpu_lib, gpu_ctx, gpu_policy):
    H.sharded_key_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy)


def test_two_contexts_meet_a_fresh_2p16_key_under_the_default_policy(gpu_lib, gpu_ctx):
    """N = 2^16 under the default policy (H_EVAL = -1) takes the evaluation basis -- read from the key's own state, not from a
    clock --, and two contexts whose first proofs start together convert it once."""
    assert gpu_lib.ctx_get_policy(gpu_ctx, "H_EVAL") == -1
    info = H.concurrent_first_proofs_case(gpu_lib, gpu_ctx, BLS12_381, (1 << 16) - 2)
    print("bind at N = 2^16: %.3f s" % info["bind_seconds"])


def test_small_key_stays_on_the_coefficient_path_by_default(gpu_lib, gpu_ctx, gpu_policy):
    """N = 2^10 under the default policy: the coefficient path (prove_csr_case checks the key's state)."""
    H.prove_csr_case(gpu_lib, gpu_ctx, BLS12_381, gpu_policy, "mulchain-1022", 0, policy_value=-1)
