"""GPU tier of the polynomial-opening entries (include/ark355.h "Polynomial openings"): the cases of tests/test_emul_poly.py on
the MI355X, plus what only the device runs in seconds: the third level of the decomposition (65 537 coefficients at one a lane,
4 194 305 at the default eight), the KZG chain on the quotient of a 5000-row Square R1CS system, and the pairing check."""
import pytest

import dirty_cases as dc
import poly_cases as pc
import sr1cs_cases as sc
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_DEFAULT)
def test_shapes_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy, C, n):
    pc.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, pc.E_DEFAULT, n)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_E1 + pc.SHAPES_E1_GPU)
def test_shapes_at_one_coefficient_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, n):
    """65 535 .. 65 537: the second level is full, then holds one chunk more -- a third level of one coefficient"""
    pc.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 1, n)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_E3)
def test_shapes_at_three_coefficients_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, n):
    pc.shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 3, n)


@CURVES
def test_policy_edge_values_never_change_a_byte(gpu_lib, gpu_ctx, gpu_policy, C):
    pc.policy_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy)


@CURVES
@pytest.mark.parametrize("count,n", [(1, 2049), (3, 2049), (5, 2049), (3, 0), (3, 1)])
def test_several_polynomials_in_one_call(gpu_lib, gpu_ctx, C, count, n):
    pc.count_case(gpu_lib, gpu_ctx, C, DevIO, count, n)


@CURVES
def test_in_place_and_refused_overlaps(gpu_lib, gpu_ctx, C):
    pc.in_place_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
@pytest.mark.parametrize("count", [0, 1, 2, 7])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2049])
def test_lincomb_against_python_sums(gpu_lib, gpu_ctx, C, count, n):
    pc.lincomb_case(gpu_lib, gpu_ctx, C, DevIO, count, n)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made"])
def test_kzg_chain_on_device_pointers(gpu_lib, gpu_ctx, C, name):
    pc.kzg_case(gpu_lib, gpu_ctx, C, DevIO, name, pairing=(C is BLS12_381))


@CURVES
def test_kzg_chain_on_a_random_sr1cs_system(gpu_lib, gpu_ctx, C):
    pc.kzg_sr1cs_case(gpu_lib, gpu_ctx, C, DevIO, *sc.random_instance(C, 5000, 0x5121C5 + C.curve_id), pairing=(C is BLS12_381))


def test_third_level_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy):
    """2048^2 + 1 coefficients: what carries the test is the byte comparison of the whole q and rem between POLY_LANE_COEFFS = 8
    and 1 and the full checks at 65 537; the recurrence in Python is a sample (poly_cases.third_level_case)"""
    pc.third_level_case(gpu_lib, gpu_ctx, BLS12_381, DevIO, gpu_policy)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        pc.dirty_sequence(gpu_lib, ctx, C, DevIO)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    pc.refusals_case(gpu_lib, gpu_ctx, C)
