"""CPU tier of the multilinear openings (include/ark355.h "Multilinear openings"): the library's own kernel and host code over the
single-threaded HIP emulator, against the big-integer reference of tests/mle_open_cases.py and the group law of oracle.curves --
the cases of tests/test_gpu_mle_open.py up to 2^14 entries for the quotients and 2^6 for the openings, plus the two tables that take
a third pass at one and two entries a lane.  The table of 2^23 entries, the opening of 2^11 entries and the pairing check are left
to the GPU tier."""
import pytest

import mle_open_cases as mo
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2], ids=["g1", "g2"])


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E8)
def test_quotients_at_the_default_decomposition(emul_lib, emul_ctx, emul_policy, C, v):
    mo.quotients_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 8, v)


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E2)
def test_quotients_at_two_entries_a_lane(emul_lib, emul_ctx, emul_policy, C, v):
    mo.quotients_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 2, v)


@CURVES
@pytest.mark.parametrize("v", mo.SHAPES_E1)
def test_quotients_at_one_entry_a_lane(emul_lib, emul_ctx, emul_policy, C, v):
    mo.quotients_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, 1, v)


@CURVES
@pytest.mark.parametrize("E,v", mo.THIRD_PASS)
def test_quotients_through_a_third_pass(emul_lib, emul_ctx, emul_policy, C, E, v):
    mo.third_pass_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy, E, v)


@CURVES
def test_policy_values_never_change_a_byte(emul_lib, emul_ctx, emul_policy, C):
    mo.policy_case(emul_lib, emul_ctx, C, sc.HostIO, emul_policy)


@CURVES
@GROUPS
@pytest.mark.parametrize("v", [0, 1, 3, 6])
def test_open_against_the_oracle_and_msm_dev(emul_lib, emul_ctx, C, group, v):
    mo.open_case(emul_lib, emul_ctx, C, sc.HostIO, group, v)


@CURVES
def test_mat_vec_sumcheck_open_chain(emul_lib, emul_ctx, C):
    mo.chain_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_overlaps_down_to_one_element(emul_lib, emul_ctx, C):
    mo.overlap_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_other_entries_between_two_opens(emul_lib, emul_ctx, C):
    mo.interleaved_case(emul_lib, emul_ctx, C, sc.HostIO)


@CURVES
def test_dirty_scratch_sequence(emul_lib, C):
    """the emulator's allocator hands out poisoned memory by itself; the context is fresh"""
    ctx = emul_lib.ctx_create(0)
    try:
        mo.dirty_sequence(emul_lib, ctx, C, sc.HostIO)
    finally:
        emul_lib.ctx_destroy(ctx)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    mo.refusals_case(emul_lib, emul_ctx, C, sc.HostIO)


def test_the_kernel_keeps_everything_in_registers():
    """tools/code_object_stats.py on the built library: mle_open_kernel of both curves, at eight entries a lane and at one, makes no
    scratch access -- a lane's eight entries and the four wave values of thread 0 are never indexed at run time"""
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
    for key in ("bls12_381.mle_open", "bn254.mle_open", "bls12_381.mle_open_e1", "bn254.mle_open_e1"):
        assert key in st, (key, sorted(st))
        assert st[key]["scratch_loads"] + st[key]["scratch_stores"] == 0, (key, st[key])
        assert st[key]["multiply_adds"] > 0, (key, st[key])
