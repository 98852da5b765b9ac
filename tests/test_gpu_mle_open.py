"""GPU tier of the multilinear openings (include/ark355.h "Multilinear openings"): the cases of tests/test_emul_mle_open.py on the
MI355X, plus what only the device finishes in seconds: a table of 2^23 entries (256 MiB in and out, a third pass at the default
eight entries a lane), an opening of 2^11 entries, and the verifier's pairing product over ark355_multi_pairing."""
import pytest

import dirty_cases as dc
import mle_open_cases as mo
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2], ids=["g1", "g2"])


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E8)
def test_quotients_at_the_default_decomposition(gpu_lib, gpu_ctx, gpu_policy, C, v):
    mo.quotients_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 8, v)


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E2)
def test_quotients_at_two_entries_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, v):
    mo.quotients_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 2, v)


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E1)
def test_quotients_at_one_entry_a_lane(gpu_lib, gpu_ctx, gpu_policy, C, v):
    mo.quotients_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 1, v)


@CURVES
@pytest.mark.parametrize("E,v", mo.THIRD_PASS)
def test_quotients_through_a_third_pass(gpu_lib, gpu_ctx, gpu_policy, C, E, v):
    mo.third_pass_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, E, v)


@CURVES
def test_two_to_the_23_through_a_third_pass_at_the_default(gpu_lib, gpu_ctx, gpu_policy, C):
    mo.large_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, 23)


@CURVES
def test_policy_values_never_change_a_byte(gpu_lib, gpu_ctx, gpu_policy, C):
    mo.policy_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy)


@CURVES
@GROUPS
@pytest.mark.parametrize("v", [0, 1, 3, 6, 11])
def test_open_against_the_oracle_and_msm_dev(gpu_lib, gpu_ctx, C, group, v):
    mo.open_case(gpu_lib, gpu_ctx, C, DevIO, group, v)


@CURVES
def test_pairing_product_of_an_opening(gpu_lib, gpu_ctx, C):
    mo.pairing_case(gpu_lib, gpu_ctx, C, DevIO, 6)


@CURVES
def test_mat_vec_sumcheck_open_chain(gpu_lib, gpu_ctx, C):
    mo.chain_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_overlaps_down_to_one_element(gpu_lib, gpu_ctx, C):
    mo.overlap_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_other_entries_between_two_opens(gpu_lib, gpu_ctx, C):
    mo.interleaved_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        mo.dirty_sequence(gpu_lib, ctx, C, DevIO)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    mo.refusals_case(gpu_lib, gpu_ctx, C, DevIO)
