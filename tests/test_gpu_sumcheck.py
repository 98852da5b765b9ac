"""GPU tier of the multilinear primitives and the sum-check of a predicate (include/ark355.h "Multilinear extensions", "Sum-check
of a GR1CS predicate"): the cases of tests/test_emul_sumcheck.py on the MI355X, rounds up to 2^13 entries, plus one run at 2^20
entries that only the device finishes in seconds."""
import pytest

import dirty_cases as dc
import sumcheck_cases as sk
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
WEIGHT = pytest.mark.parametrize("weight", [True, False], ids=["weight", "no-weight"])


@CURVES
@pytest.mark.parametrize("v", sk.MLE_SHAPES_DEFAULT)
def test_primitives_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy, C, v):
    sk.primitives_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, sk.P_DEFAULT, v)


@CURVES
@pytest.mark.parametrize("v", sk.MLE_SHAPES_P2)
def test_primitives_at_two_elements_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, v):
    sk.primitives_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 2, v)


@CURVES
def test_primitives_on_five_tables(gpu_lib, gpu_ctx, gpu_policy, C):
    sk.primitives_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, sk.P_DEFAULT, 5, counts=(5,))


@CURVES
def test_eval_is_linear_through_lincomb(gpu_lib, gpu_ctx, C):
    sk.lincomb_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
@WEIGHT
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_DEFAULT + (12, 13))
def test_rounds_r1cs_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy, C, v, weight):
    sk.rounds_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, sk.P_DEFAULT, "r1cs", v, weight)


@CURVES
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_P2)
def test_rounds_r1cs_at_two_pairs_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, v):
    sk.rounds_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 2, "r1cs", v, True)


@CURVES
@pytest.mark.parametrize("v", sk.ROUND_SHAPES_P3)
def test_rounds_r1cs_at_three_pairs_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, v):
    sk.rounds_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 3, "r1cs", v, True)


@CURVES
@WEIGHT
@pytest.mark.parametrize("name", ["sr1cs", "arity1", "deg3", "deg5", "deg1", "deg0", "arity16", "zero-top"])
@pytest.mark.parametrize("v", [0, 1, 2, 3, 7])
def test_rounds_of_every_predicate(gpu_lib, gpu_ctx, gpu_policy, C, name, v, weight):
    sk.rounds_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, sk.P_DEFAULT, name, v, weight)


@CURVES
@pytest.mark.parametrize("name,weight", [("deg31", False), ("deg30", True)])
@pytest.mark.parametrize("v", [1, 6])
def test_rounds_of_exactly_32_points(gpu_lib, gpu_ctx, gpu_policy, C, name, weight, v):
    sk.rounds_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, sk.P_DEFAULT, name, v, weight)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-N8"])
def test_mat_vec_output_satisfied_and_broken(gpu_lib, gpu_ctx, C, name):
    sk.system_case(gpu_lib, gpu_ctx, C, DevIO, name)


@CURVES
@pytest.mark.parametrize("name,v,weight", [("r1cs", 6, True), ("deg3", 4, False), ("r1cs", 10, True)])
def test_restart_from_folded_tables(gpu_lib, gpu_ctx, C, name, v, weight):
    sk.restart_case(gpu_lib, gpu_ctx, C, DevIO, name, v, weight)


@CURVES
def test_policy_values_never_change_a_byte(gpu_lib, gpu_ctx, gpu_policy, C):
    sk.policy_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy)


@CURVES
def test_other_entries_between_rounds(gpu_lib, gpu_ctx, C):
    sk.interleaved_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_calls_out_of_order(gpu_lib, gpu_ctx, C):
    sk.order_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_two_to_the_20_with_a_second_reduction_level(gpu_lib, gpu_ctx, gpu_policy, C):
    """The R1CS shape with a weight takes 10 LDS slots a lane, so a workgroup of the round kernel has 128 lanes.  At one pair a lane
    round 1 of N entries runs N / 256 workgroups, and the sum kernel adds 2048 partials a workgroup: the partial reduction takes a
    second level from N = 2^20 on (4096 workgroups -> 2 -> 1), which is this case at SUMCHECK_LANE_PAIRS = 1, the default since the
    measurements; four pairs a lane (1024 workgroups, one level) is the other side of the byte comparison.  2^20 is above 2^13: the
    emulator tier does not reach it."""
    sk.large_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 20)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        sk.dirty_sequence(gpu_lib, ctx, C, DevIO)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    sk.refusals_case(gpu_lib, gpu_ctx, C)
