"""CPU tier of the multilinear primitives and the sum-check of a predicate (include/ark355.h "Multilinear extensions", "Sum-check
of a GR1CS predicate"): the library's own kernels and host code over the single-threaded HIP emulator, against the big-integer
reference and verifier of tests/sumcheck_cases.py -- the cases of tests/test_gpu_sumcheck.py up to 2^13 entries for the primitives
and 2^12 for the rounds.  The second level of the partial reduction needs more than 2048 workgroups (2^20 entries at one pair a
lane for the R1CS shape) and is left to the GPU tier."""
import pytest

import sr1cs_cases as sc
import sumcheck_cases as sk
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
WEIGHT = pytest.mark.parametrize("weight", [True, False], ids=["weight", "no-weight"])


@CURVES
@pytest.mark.parametrize("v", sk.MLE_SHAPES_DEFAULT)
def test_primitives_at_the_default_decomposition(emul_lib, emul_ctx, emul_policy, C, v):
    sk.primitives_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, sk.P_DEFAULT, v)


@CURVES
@pytest.mark.parametrize("v", sk.MLE_SHAPES_P2)
def test_primitives_at_two_elements_a_lane(emul_lib, emul_ctx, emul_policy, C, v):
    sk.primitives_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 2, v)


@CURVES
def test_primitives_on_five_tables(emul_lib, emul_ctx, emul_policy, C):
    sk.primitives_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, sk.P_DEFAULT, 5, counts=(5,))


@CURVES
def test_eval_is_linear_through_lincomb(emul_lib, emul_ctx, C):
    sk.lincomb_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
@WEIGHT
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_DEFAULT + (12,))
def test_rounds_r1cs_at_the_default_decomposition(emul_lib, emul_ctx, emul_policy, C, v, weight):
    sk.rounds_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, sk.P_DEFAULT, "r1cs", v, weight)


@CURVES
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_P2)
def test_rounds_r1cs_at_two_pairs_a_lane(emul_lib, emul_ctx, emul_policy, C, v):
    sk.rounds_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 2, "r1cs", v, True)


@CURVES
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_P3)
def test_rounds_r1cs_at_three_pairs_a_lane(emul_lib, emul_ctx, emul_policy, C, v):
    sk.rounds_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 3, "r1cs", v, True)


@CURVES
@WEIGHT
@pytest.mark.parametrize("name", ["sr1cs", "arity1", "deg3", "deg5", "deg1", "deg0", "arity16", "zero-top"])
@pytest.mark.parametrize("v", [0, 1, 2, 3, 7])
def test_rounds_of_every_predicate(emul_lib, emul_ctx, emul_policy, C, name, v, weight):
    sk.rounds_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, sk.P_DEFAULT, name, v, weight)


@CURVES
@pytest.mark.parametrize("name,weight", [("deg31", False), ("deg30", True)])
@pytest.mark.parametrize("v", [1, 6])
def test_rounds_of_exactly_32_points(emul_lib, emul_ctx, emul_policy, C, name, weight, v):
    sk.rounds_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, sk.P_DEFAULT, name, v, weight)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-N8"])
def test_mat_vec_output_satisfied_and_broken(emul_lib, emul_ctx, C, name):
    sk.system_case(emul_lib, emul_ctx, C, sc.HostIO, name)


@CURVES
@pytest.mark.parametrize("name,v,weight", [("r1cs", 6, True), ("deg3", 4, False), ("r1cs", 10, True)])
def test_restart_from_folded_tables(emul_lib, emul_ctx, C, name, v, weight):
    sk.restart_case(emul_lib, emul_ctx, C, sc.HostIO, name, v, weight)


@CURVES
def test_policy_values_never_change_a_byte(emul_lib, emul_ctx, emul_policy, C):
    sk.policy_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy)


@CURVES
def test_other_entries_between_rounds(emul_lib, emul_ctx, C):
    sk.interleaved_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_calls_out_of_order(emul_lib, emul_ctx, C):
    sk.order_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        sk.dirty_sequence(emul_lib, ctx, C, sc.HostIO)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    sk.refusals_case(emul_lib, emul_ctx, C)
