"""CPU tier of the batched short MSMs (include/ark355.h "Batched short MSMs"): the library's own kernel and host code over the
single-threaded HIP emulator, against the group law of oracle.curves, ark355_msm_dev segment by segment and the same batch with the
short route switched off (tests/msm_batch_cases.py).  The batches of thousands of segments, the segment of 2^15 scalars, the
opening of 2^14 entries and 1024 scalars under every plan are left to the GPU tier."""
import pytest

import msm_batch_cases as mb
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2], ids=["g1", "g2"])
PLANS = pytest.mark.parametrize("nb,c,stride,pack", mb.PLANS)
# Every plan runs 5 and 64 scalars on both curves and groups; the segment of 1024 scalars -- 131 072 emulated additions, up to a
# minute on lane pairs -- joins where a path of its own is at stake: the smallest window, the negated scalars of BLS12-381 at 17
# bits, and a stride on lane pairs.  The GPU tier runs 1024 scalars under every plan.
LONG_PLANS = {("bn254", 1, 1024, 4, 1, 0), ("bls12_381", 1, 1024, 17, 2, 0), ("bn254", 2, 1024, 8, 2, 1)}


@pytest.mark.parametrize("C,group,use_mont", [(BLS12_381, 1, 0), (BLS12_381, 2, 1), (BN254, 1, 1), (BN254, 2, 0)],
                         ids=["bls12_381-g1-canonical", "bls12_381-g2-montgomery", "bn254-g1-montgomery", "bn254-g2-canonical"])
def test_every_length_in_one_batch(emul_lib, emul_ctx, emul_policy, C, group, use_mont):
    """each curve and group once; canonical and Montgomery scalars on either group (the GPU tier runs all eight)"""
    mb.lengths_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group, use_mont)


@CURVES
@GROUPS
def test_the_shape_of_an_opening(emul_lib, emul_ctx, emul_policy, C, group):
    mb.opening_shape_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group, top=10 if group == 1 else 8)


@CURVES
@GROUPS
def test_one_handle_64_times(emul_lib, emul_ctx, emul_policy, C, group):
    mb.repeated_handle_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group, n=4)


@CURVES
@GROUPS
def test_equal_opposite_and_empty_bases(emul_lib, emul_ctx, emul_policy, C, group):
    mb.designed_bases_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group)


@CURVES
@GROUPS
@PLANS
def test_handles_of_other_plans(emul_lib, emul_ctx, emul_policy, C, group, nb, c, stride, pack):
    long_too = (C.name, group, nb, c, stride, pack) in LONG_PLANS
    mb.plan_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group, nb, c, stride, pack, mb.PLAN_LENGTHS if long_too else mb.PLAN_LENGTHS[:2])


@CURVES
@GROUPS
def test_policy_values_never_change_a_byte(emul_lib, emul_ctx, emul_policy, C, group):
    mb.policy_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group)


@CURVES
@GROUPS
def test_open_dev_is_the_same_on_both_routes(emul_lib, emul_ctx, emul_policy, C, group):
    mb.open_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, group, 6)


@CURVES
@GROUPS
def test_commit_dev_against_msm_dev(emul_lib, emul_ctx, C, group):
    mb.commit_case(emul_lib, emul_ctx, C, sc.HostIO, group)


@CURVES
def test_other_entries_between_two_batches(emul_lib, emul_ctx, C):
    mb.interleaved_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        mb.dirty_sequence(emul_lib, ctx, C, sc.HostIO)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    mb.refusals_case(emul_lib, emul_ctx, C, sc.HostIO)


def test_the_sum_kernels_keep_everything_in_registers():
    """tools/code_object_stats.py on the built library: the sum kernel of both curves, both groups and both row formats makes no
    scratch access and does multiply -- not in its loops, and not on the cold paths of the group law either, whose operands travel
    in registers (MsmBatchCold)"""
    import os
    import sys
    from snark_amd import build
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import code_object_stats as cos
        st = cos.library_stats(build.build(verbose=False))
    finally:
        sys.path.remove(os.path.join(root, "tools"))
    for curve in ("bls12_381", "bn254"):
        for kind in ("g1", "g1_packed", "g2", "g2_packed"):
            key = "%s.msm_batch_sum_%s" % (curve, kind)
            assert key in st, (key, sorted(st))
            assert st[key]["scratch_loads"] + st[key]["scratch_stores"] == 0, (key, st[key])
            assert st[key]["multiply_adds"] > 0, (key, st[key])
