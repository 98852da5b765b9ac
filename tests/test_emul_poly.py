"""CPU tier of the polynomial-opening entries (include/ark355.h "Polynomial openings"): the library's own kernels and host code
over the single-threaded HIP emulator, against the references of tests/poly_cases.py -- the cases of tests/test_gpu_poly.py
up to two levels of the decomposition (4097 coefficients at eight a lane, 513 at one)."""
import pytest

import poly_cases as pc
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_DEFAULT)
def test_shapes_at_the_default_decomposition(emul_lib, emul_ctx, emul_policy, C, n):
    pc.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, pc.E_DEFAULT, n)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_E1)
def test_shapes_at_one_coefficient_a_lane(emul_lib, emul_ctx, emul_policy, C, n):
    pc.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 1, n)


@CURVES
@pytest.mark.parametrize("n", pc.SHAPES_E3)
def test_shapes_at_three_coefficients_a_lane(emul_lib, emul_ctx, emul_policy, C, n):
    pc.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 3, n)


@CURVES
def test_policy_edge_values_never_change_a_byte(emul_lib, emul_ctx, emul_policy, C):
    pc.policy_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy)


@CURVES
@pytest.mark.parametrize("count,n", [(1, 2049), (3, 2049), (5, 2049), (3, 0), (3, 1)])
def test_several_polynomials_in_one_call(emul_lib, emul_ctx, C, count, n):
    pc.count_case(emul_lib, emul_ctx, C, sc.HostIO, count, n)


@CURVES
def test_in_place_and_refused_overlaps(emul_lib, emul_ctx, C):
    pc.in_place_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
@pytest.mark.parametrize("count", [0, 1, 2, 7])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2049])
def test_lincomb_against_python_sums(emul_lib, emul_ctx, C, count, n):
    pc.lincomb_case(emul_lib, emul_ctx, C, sc.HostIO, count, n)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made"])
def test_kzg_chain_on_device_pointers(emul_lib, emul_ctx, C, name):
    pc.kzg_case(emul_lib, emul_ctx, C, sc.HostIO, name)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        pc.dirty_sequence(emul_lib, ctx, C, sc.HostIO)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    pc.refusals_case(emul_lib, emul_ctx, C)
