"""CPU tier of the column-polynomial entries (include/ark355.h "Column polynomials of any predicate at a point"): the library's
own kernels and host code over the single-threaded HIP emulator, against the references of tests/columns_cases.py -- the cases
of tests/test_gpu_columns.py at sizes the emulator runs in seconds."""
import pytest

import columns_cases as cc
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
SR1CS_INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


@CURVES
@pytest.mark.parametrize("arity", [1, 2, 3, 4, 16])
def test_mat_vec_t_by_arity(emul_lib, emul_ctx, C, arity):
    cc.arity_case(emul_lib, emul_ctx, C, arity)


@CURVES
def test_mat_vec_t_edges(emul_lib, emul_ctx, C):
    cc.edges_case(emul_lib, emul_ctx, C)


@CURVES
def test_several_predicates_by_the_callers_index(emul_lib, emul_ctx, C):
    cc.several_predicates_case(emul_lib, emul_ctx, C)


@CURVES
def test_column_lengths_around_both_thresholds(emul_lib, emul_ctx, emul_policy, C):
    cc.lengths_case(emul_lib, emul_ctx, C, emul_policy)


@CURVES
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 10])
def test_lagrange_fr(emul_lib, emul_ctx, C, log_n):
    cc.lagrange_case(emul_lib, emul_ctx, C, log_n)


@CURVES
def test_columns_at_against_the_sums(emul_lib, emul_ctx, C):
    cc.columns_at_case(emul_lib, emul_ctx, C)


@CURVES
@pytest.mark.parametrize("n", [13, 1030])
def test_columns_at_equals_the_generators_u_v_w(emul_lib, emul_ctx, C, n):
    cc.setup_case(emul_lib, emul_ctx, C, n)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-arity4-N8"])
def test_qap_identity_at_a_point(emul_lib, emul_ctx, C, name):
    cc.qap_case(emul_lib, emul_ctx, C, name)


@CURVES
@pytest.mark.parametrize("which", range(len(SR1CS_INSTANCES)), ids=SR1CS_INSTANCES)
def test_sr1cs_chain_on_device_pointers(emul_lib, emul_ctx, C, which):
    cc.sr1cs_chain_case(emul_lib, emul_ctx, C, sc.HostIO, *sc.reference_instances(C)[which])


@CURVES
def test_handle_from_lcs(emul_lib, emul_ctx, C):
    cc.from_lcs_case(emul_lib, emul_ctx, C)


@CURVES
def test_dev_variants(emul_lib, emul_ctx, C):
    cc.dev_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
@pytest.mark.parametrize("group,n", [(1, 5), (2, 5), (1, cc.FB_TABLE_MIN + 8)], ids=["g1-5", "g2-5", "g1-table"])
def test_fixed_base_mul_dev(emul_lib, emul_ctx, C, group, n):
    cc.fixed_base_case(emul_lib, emul_ctx, C, sc.HostIO, group, n)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        cc.dirty_sequence(emul_lib, ctx, C)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    cc.refusals_case(emul_lib, emul_ctx, C)
