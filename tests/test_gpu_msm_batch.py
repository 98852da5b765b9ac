"""GPU tier of the batched short MSMs (include/ark355.h "Batched short MSMs"): the cases of tests/test_emul_msm_batch.py on the
MI355X, plus what only the device finishes in seconds: 4096 segments of 16 scalars, 64 segments of 1024, a segment of 2^15 scalars
between short ones, and an opening of 2^14 entries on both routes."""
import pytest

import dirty_cases as dc
import msm_batch_cases as mb
from test_gpu_quotient import DevIO
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2], ids=["g1", "g2"])
PLANS = pytest.mark.parametrize("nb,c,stride,pack", mb.PLANS)


@CURVES
@GROUPS
@pytest.mark.parametrize("use_mont", [0, 1], ids=["canonical", "montgomery"])
def test_every_length_in_one_batch(gpu_lib, gpu_ctx, gpu_policy, C, group, use_mont):
    mb.lengths_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group, use_mont)


@CURVES
@GROUPS
def test_the_shape_of_an_opening(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.opening_shape_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group)


@CURVES
@GROUPS
def test_one_handle_64_times(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.repeated_handle_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group)


@CURVES
@GROUPS
def test_equal_opposite_and_empty_bases(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.designed_bases_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group)


@CURVES
@GROUPS
@PLANS
def test_handles_of_other_plans(gpu_lib, gpu_ctx, gpu_policy, C, group, nb, c, stride, pack):
    mb.plan_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group, nb, c, stride, pack)


@CURVES
@GROUPS
def test_policy_values_never_change_a_byte(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.policy_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group)


@CURVES
@GROUPS
@pytest.mark.parametrize("v", [6, 11, 14])
def test_open_dev_is_the_same_on_both_routes(gpu_lib, gpu_ctx, gpu_policy, C, group, v):
    mb.open_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group, v)


@CURVES
@GROUPS
def test_commit_dev_against_msm_dev(gpu_lib, gpu_ctx, C, group):
    mb.commit_case(gpu_lib, gpu_ctx, C, DevIO, group)


@CURVES
@GROUPS
def test_4096_segments_of_16(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.many_segments_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group, 4096, 16)


@CURVES
@GROUPS
def test_64_segments_of_1024(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.many_segments_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group, 64, 1024)


@CURVES
@GROUPS
def test_a_long_segment_between_short_ones(gpu_lib, gpu_ctx, gpu_policy, C, group):
    mb.long_between_short_case(gpu_lib, gpu_ctx, C, DevIO, gpu_policy, group)


@CURVES
def test_other_entries_between_two_batches(gpu_lib, gpu_ctx, C):
    mb.interleaved_case(gpu_lib, gpu_ctx, C, DevIO)


@CURVES
def test_dirty_scratch_sequence(gpu_lib, C):
    """one fresh context created with POISON_ALLOC set, as tests/dirty_cases.py sets it up"""
    ctx = dc.fresh_context(gpu_lib)
    try:
        mb.dirty_sequence(gpu_lib, ctx, C, DevIO)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    mb.refusals_case(gpu_lib, gpu_ctx, C, DevIO)
