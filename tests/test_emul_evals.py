"""CPU tier of the openings in the evaluation basis (include/ark355.h "Openings in the evaluation basis"): the library's own kernels
and host code over the single-threaded HIP emulator, against the three references of tests/evals_cases.py -- the cases of
tests/test_gpu_evals.py up to 2^13 points (four workgroups at eight points a lane, two launches of the sum kernel)."""
import pytest

import evals_cases as ec
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_DEFAULT)
def test_shapes_at_the_default_decomposition(emul_lib, emul_ctx, emul_policy, C, log_n):
    ec.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, ec.E_DEFAULT, log_n)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_E1)
def test_shapes_at_one_point_a_lane(emul_lib, emul_ctx, emul_policy, C, log_n):
    ec.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 1, log_n)


@CURVES
@pytest.mark.parametrize("log_n", ec.SHAPES_E3)
def test_shapes_at_three_points_a_lane(emul_lib, emul_ctx, emul_policy, C, log_n):
    ec.shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 3, log_n)


@CURVES
def test_policy_values_never_change_a_byte(emul_lib, emul_ctx, emul_policy, C):
    ec.policy_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy)


@CURVES
@pytest.mark.parametrize("count,log_n", [(1, 12), (3, 12), (5, 12), (3, 0)])
def test_several_vectors_in_one_call(emul_lib, emul_ctx, C, count, log_n):
    ec.count_case(emul_lib, emul_ctx, C, sc.HostIO, count, log_n)


@CURVES
def test_in_place_and_refused_overlaps(emul_lib, emul_ctx, C):
    ec.in_place_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "sr1cs"])
def test_mat_vec_dev(emul_lib, emul_ctx, C, name):
    ec.mat_vec_case(emul_lib, emul_ctx, C, sc.HostIO, name)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made"])
def test_chain_on_device_pointers_with_a_lagrange_key(emul_lib, emul_ctx, C, name):
    ec.chain_case(emul_lib, emul_ctx, C, sc.HostIO, name)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        ec.dirty_sequence(emul_lib, ctx, C, sc.HostIO)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    ec.refusals_case(emul_lib, emul_ctx, C)
