"""CPU tier of the h query in the evaluation basis (policy H_EVAL; snark_amd/csrc/hbasis_impl.cuh): the library's own sources
against the HIP emulator, cases and references in tests/hbasis_cases.py."""
import pytest

import hbasis_cases as H
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
@pytest.mark.parametrize("log_n", [1, 3, 6])
def test_group_transforms_vs_direct_sums(emul_lib, emul_ctx, C, log_n):
    H.transform_case(emul_lib, emul_ctx, C, log_n)


@CURVES
def test_group_transform_with_infinity_inside(emul_lib, emul_ctx, C):
    """H_2 and H_5 at infinity (index N - 1 always is)."""
    H.transform_case(emul_lib, emul_ctx, C, 3, inf_at=(2, 5))


@CURVES
def test_gather_hand_built_columns(emul_lib, emul_ctx, C):
    H.gather_hand_built_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("n", [(1 << 11) + 1, (1 << 11) + 2], ids=["one-full-chunk", "two-chunks"])
def test_gather_heavy_column(emul_lib, emul_ctx, n):
    H.gather_heavy_case(emul_lib, emul_ctx, BLS12_381, n)


@CURVES
def test_gather_column_lengths(emul_lib, emul_ctx, C):
    """columns of 63, 64, 65, 2048, 2049 and 0 entries: both sides of the lane limit and of the chunk, with scalar multiplications"""
    H.gather_lengths_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("h_eval", [1, 0], ids=["H_EVAL=1", "H_EVAL=0"])
@pytest.mark.parametrize("name", ["mulchain-6", "mulchain-32", "golden", "ell1"])
def test_proofs_match_the_oracle_on_both_paths(emul_lib, emul_ctx, emul_policy, name, h_eval):
    H.prove_rows_case(emul_lib, emul_ctx, BLS12_381, emul_policy, name, h_eval)


@pytest.mark.parametrize("h_eval", [1, 0], ids=["H_EVAL=1", "H_EVAL=0"])
def test_proofs_bn254(emul_lib, emul_ctx, emul_policy, h_eval):
    H.prove_rows_case(emul_lib, emul_ctx, BN254, emul_policy, "mulchain-6", h_eval)


@pytest.mark.parametrize("h_eval", [1, 0], ids=["H_EVAL=1", "H_EVAL=0"])
@pytest.mark.parametrize("name", ["mulchain-1022", "dummy-256"])
def test_proofs_match_oracle_c_on_both_paths(emul_lib, emul_ctx, emul_policy, name, h_eval):
    """mulchain at n = 2^10 - 2: N = 2^10, the smallest domain with the fused inverse -> coset seam; the DummyCircuit at 2^8."""
    H.prove_csr_case(emul_lib, emul_ctx, BLS12_381, emul_policy, name, h_eval)


@pytest.mark.parametrize("h_eval", [1, 0], ids=["H_EVAL=1", "H_EVAL=0"])
def test_unsatisfied_assignment_proves_like_the_seven_transform_prover(emul_lib, emul_ctx, emul_policy, h_eval):
    H.prove_rows_case(emul_lib, emul_ctx, BLS12_381, emul_policy, "mulchain-6", h_eval, unsatisfied=True)


def test_check_satisfied_on_a_bound_key(emul_lib, emul_ctx, emul_policy):
    H.check_satisfied_case(emul_lib, emul_ctx, BLS12_381, emul_policy)


def test_bound_key_refuses_another_r1cs_handle(emul_lib, emul_ctx, emul_policy):
    H.other_r1cs_refused_case(emul_lib, emul_ctx, BLS12_381, emul_policy)


def test_policy_default_and_small_keys_stay_on_the_coefficient_path(emul_lib, emul_ctx):
    """H_EVAL defaults to -1 (evaluation basis from N = 2^16 on): a small key settles on the coefficient path at its first proof."""
    import parity_cases as pc
    from oracle import synthetic as S
    assert emul_lib.ctx_get_policy(emul_ctx, "H_EVAL") == -1
    C = BLS12_381
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 6)
    pc.prove_case(emul_lib, emul_ctx, C, A, B, Cm, z, ell)


def test_key_shards_keep_the_coefficient_path(emul_lib, emul_ctx, emul_policy):
    H.sharded_key_case(emul_lib, emul_ctx, BLS12_381, emul_policy)
