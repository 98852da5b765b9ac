"""GPU tier of the column-polynomial entries (include/ark355.h "Column polynomials of any predicate at a point"): the cases of
tests/test_emul_columns.py on the MI355X, plus what only the device runs in seconds: Lagrange vectors of 2^13 points, the
generator's u, v, w at 2^14 and 2^18 rows, the SR1CS chain at 5000 source rows, the table path of the fixed-base
multiplication in G2, and matrices -> key scalars -> key points without the host."""
import pytest

import columns_cases as cc
import dirty_cases as dc
import sr1cs_cases as sc
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
SR1CS_INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


@CURVES
@pytest.mark.parametrize("arity", [1, 2, 3, 4, 16])
def test_mat_vec_t_by_arity(gpu_lib, gpu_ctx, C, arity):
    cc.arity_case(gpu_lib, gpu_ctx, C, arity)


@CURVES
def test_mat_vec_t_edges(gpu_lib, gpu_ctx, C):
    cc.edges_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_several_predicates_by_the_callers_index(gpu_lib, gpu_ctx, C):
    cc.several_predicates_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_column_lengths_around_both_thresholds(gpu_lib, gpu_ctx, gpu_policy, C):
    cc.lengths_case(gpu_lib, gpu_ctx, C, gpu_policy)


@CURVES
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 10, 13])
def test_lagrange_fr(gpu_lib, gpu_ctx, C, log_n):
    """a lane owns eight consecutive points: 1, 2 and 4 points are partial runs, 2^13 points are four workgroups"""
    cc.lagrange_case(gpu_lib, gpu_ctx, C, log_n)


@CURVES
def test_columns_at_against_the_sums(gpu_lib, gpu_ctx, C):
    cc.columns_at_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_columns_at_equals_the_generators_u_v_w(gpu_lib, gpu_ctx, C):
    cc.setup_case(gpu_lib, gpu_ctx, C, 1 << 14)


def test_columns_at_equals_the_generators_u_v_w_at_two_to_the_eighteen(gpu_lib, gpu_ctx):
    from test_gpu_sr1cs import bench_lc_shape
    C = BLS12_381
    ell, w, mats, z = bench_lc_shape(C.r, 1 << 18)
    cc.setup_csr_case(gpu_lib, gpu_ctx, C, ell, w, mats)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-arity4-N8"])
def test_qap_identity_at_a_point(gpu_lib, gpu_ctx, C, name):
    cc.qap_case(gpu_lib, gpu_ctx, C, name)


@CURVES
@pytest.mark.parametrize("which", range(len(SR1CS_INSTANCES)), ids=SR1CS_INSTANCES)
def test_sr1cs_chain_on_device_pointers(gpu_lib, gpu_ctx, C, which):
    cc.sr1cs_chain_case(gpu_lib, gpu_ctx, C, DevIO, *sc.reference_instances(C)[which])


@CURVES
def test_sr1cs_chain_on_a_random_system(gpu_lib, gpu_ctx, C):
    cc.sr1cs_chain_case(gpu_lib, gpu_ctx, C, DevIO, *sc.random_instance(C, 5000, 0x5121C5 + C.curve_id))


@CURVES
def test_handle_from_lcs(gpu_lib, gpu_ctx, C):
    cc.from_lcs_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_dev_variants(gpu_lib, gpu_ctx, C):
    cc.dev_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [5, cc.FB_TABLE_MIN - 1, cc.FB_TABLE_MIN + 8])
def test_fixed_base_mul_dev(gpu_lib, gpu_ctx, C, group, n):
    cc.fixed_base_case(gpu_lib, gpu_ctx, C, DevIO, group, n)


@CURVES
def test_matrices_to_key_points_without_the_host(gpu_lib, gpu_ctx, C):
    cc.key_points_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        cc.dirty_sequence(gpu_lib, ctx, C)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    cc.refusals_case(gpu_lib, gpu_ctx, C)
