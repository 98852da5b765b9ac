"""GPU tier of the openings in the evaluation basis (include/ark355.h "Openings in the evaluation basis"): the cases of
tests/test_emul_evals.py on the MI355X, plus what only the device runs in seconds: the chain on a 5000-row Square R1CS system with
the pairing check, the second level of the sum kernel (more than 2048 workgroups: 2^20 and 2^21 points at one point a lane) and
2^22 points against the coefficient route on device pointers."""
import pytest

import dirty_cases as dc
import evals_cases as ec
import sr1cs_cases as sc
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_DEFAULT)
def test_shapes_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy, C, log_n):
    ec.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, ec.E_DEFAULT, log_n)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_E1)
def test_shapes_at_one_point_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, log_n):
    ec.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 1, log_n)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_E3)
def test_shapes_at_three_points_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, log_n):
    ec.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 3, log_n)


@CURVES
def test_policy_values_never_change_a_byte(gpu_lib, gpu_ctx, gpu_policy, C):
    ec.policy_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy)


@CURVES
@pytest.mark.parametrize("count,log_n", [(1, 12), (3, 12), (5, 12), (3, 0)])
def test_several_vectors_in_one_call(gpu_lib, gpu_ctx, C, count, log_n):
    ec.count_case(gpu_lib, gpu_ctx, C, DevIO, count, log_n)


@CURVES
def test_in_place_and_refused_overlaps(gpu_lib, gpu_ctx, C):
    ec.in_place_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "sr1cs"])
def test_mat_vec_dev(gpu_lib, gpu_ctx, C, name):
    ec.mat_vec_case(gpu_lib, gpu_ctx, C, DevIO, name)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made"])
def test_chain_on_device_pointers_with_a_lagrange_key(gpu_lib, gpu_ctx, C, name):
    ec.chain_case(gpu_lib, gpu_ctx, C, DevIO, name, pairing=(C is BLS12_381))


@CURVES
def test_chain_on_a_random_sr1cs_system(gpu_lib, gpu_ctx, C):
    ec.chain_sr1cs_case(gpu_lib, gpu_ctx, C, DevIO, *sc.random_instance(C, 5000, 0x5121C5 + C.curve_id), pairing=(C is BLS12_381))


@CURVES
@pytest.mark.parametrize("log_n", [20, 21])
def test_second_level_of_the_sum_kernel(gpu_lib, gpu_ctx, gpu_policy, C, log_n):
    """at one point a lane 2^20 points are 4096 workgroups: the sum kernel runs a second level, 4096 -> 2 -> 1; the default (512
    and 1024 workgroups, one level) is the other decomposition of the byte comparison"""
    ec.large_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, log_n, 1, j_frac=0.75, samples=512)


@CURVES
def test_two_to_the_22_against_the_coefficient_route(gpu_lib, gpu_ctx, gpu_policy, C):
    """x outside the domain and x = a_j in the last workgroup; q and y byte-identical to the coefficient route on the device,
    the identity at 4096 random indices, EVALS_LANE_POINTS = 8 against 1"""
    ec.large_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 22, 1)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        ec.dirty_sequence(gpu_lib, ctx, C, DevIO)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    ec.refusals_case(gpu_lib, gpu_ctx, C)
