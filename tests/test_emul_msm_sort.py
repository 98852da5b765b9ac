"""CPU tier: the sort stage of the MSMs on the emulator build, through ark355_diag_msm_sort, against the plain-integer reference
of tests/msm_sort_cases.py -- signed digits, histogram, scan and placement checked on their own, so that a failure names the
stage and not just "wrong point".

The emulator build keeps 256 first-level bins in "LDS" (ARK_SORT_MAX_BINS; the product keeps 4096), so 2^17 buckets -- window
17 over tables for every second window -- take the one-pass counting sort with its wave-aggregated atomics, which the product
reaches above 2^20 buckets.  GPU twin: tests/test_gpu_msm_sort.py."""
import numpy as np
import pytest

import msm_sort_cases as mc
import parity_cases as pc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254

CURVES = [BLS12_381, BN254]
ROWS = 1100            # resident shapes: the policy's window size applies from 1024 rows on
TIER_WINDOWS = (4, 5, 8, 13, 15, 16, 17, 18, 20, 22, 24)       # every window size either tier sorts with


def _to_dev(b):        # emulator: "device" pointers are host pointers
    a = np.frombuffer(b, dtype=np.uint8).copy()
    return a.ctypes.data, a


@pytest.fixture(scope="module")
def bases(emul_lib, emul_ctx):
    cache = mc.BasesCache(emul_lib, emul_ctx)
    yield cache
    cache.close()


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("c", TIER_WINDOWS)
def test_reference_digits_recompose(C, c):
    """The reference checks itself: over the edge set of every window size used by either tier, with and without the negation of
    high scalars, the signed digits stay in [0, 2^(c-1)], the top window does not carry out, and sum +-d_w 2^(c w) == k mod r."""
    for resident in (False, True):
        plan = mc.expected_plan(C, c, resident, 1, ROWS)
        B = 1 << (c - 1)
        seen_half = seen_zero_carry = False
        for k in mc.edge_scalars(C.r, c, plan["windows"]) + mc.scalar_set("uniform", C.r, c, plan["windows"], 50):
            ds, negs = mc.scalar_digits(k, C.r, c, plan["windows"], plan["negate_high"])       # asserts the recomposition
            assert len(ds) == plan["windows"] and all(0 <= d <= B for d in ds)
            seen_half |= B in ds
            seen_zero_carry |= any(d == 0 and s for d, s in zip(ds, negs))
        assert seen_half and seen_zero_carry             # the edge set reaches d == 2^(c-1) and a zero digit that carries
    assert mc.signed_digits(B, c, 2) == ([B, 0], [0, 0])                       # exactly 2^(c-1): positive, no carry
    assert mc.signed_digits(B + 1, c, 2) == ([B - 1, 1], [1, 0])
    assert mc.signed_digits((1 << (2 * c)) - 1, c, 3) == ([1, 0, 1], [1, 1, 0])     # a zero digit that still carries


def test_reference_window_counts():
    """The plan the reference derives, at the shapes DESIGN.md quotes: 16 / 15 windows at c = 16 / 17 over 255 bits (the negation
    saves one), 15 without negation over BN254's 254 bits, 13 at c = 20; one-shot windows 4 / 8 / 13 by length."""
    assert mc.expected_plan(BLS12_381, 16, True)["windows"] == 16 and mc.expected_plan(BLS12_381, 16, True)["negate_high"] == 0
    assert mc.expected_plan(BLS12_381, 17, True)["windows"] == 15 and mc.expected_plan(BLS12_381, 17, True)["negate_high"] == 1
    assert mc.expected_plan(BN254, 17, True)["windows"] == 15 and mc.expected_plan(BN254, 17, True)["negate_high"] == 0
    assert mc.expected_plan(BLS12_381, 20, True)["windows"] == 13 and mc.expected_plan(BLS12_381, 5, True)["windows"] == 51
    assert mc.expected_plan(BLS12_381, 17, False)["windows"] == 16
    assert [mc.oneshot_window(n, 255) for n in (1, 300, 4096, 8197, 1 << 15)] == [4, 4, 8, 8, 13]
    assert [mc.oneshot_window(n, 254) for n in (1, 300, 4096, 8197, 1 << 15)] == [5, 5, 8, 8, 13]


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_sort_one_shot(emul_lib, emul_ctx, C, n):
    """The plan without tables (every window its own bucket set): a single scalar, partial and whole waves, more than one
    workgroup of the digit kernels; every scalar set; Montgomery scalars at the wave boundary."""
    mc.sort_case(emul_lib, emul_ctx, C, n, mc.SETS, mont=(0, 1) if n == 65 else (0,), one_pass=False)


@pytest.mark.parametrize("C,c", [(BLS12_381, 5), (BLS12_381, 8), (BLS12_381, 13), (BLS12_381, 15), (BLS12_381, 17),
                                 (BN254, 8), (BN254, 17)], ids=lambda v: getattr(v, "name", str(v)))
def test_sort_resident(emul_lib, emul_ctx, bases, C, c):
    """Window tables, one bucket set: c = 5, 15, 17 negate the scalars above (r - 1) / 2 on BLS12-381; BN254 at c = 17 is the exact
    fit of 254 bits + carry in 15 windows; 2^14 buckets (c = 15) is the last single-tile scan of the emulator build, 2^16 the
    split scan over four spans."""
    h = bases.get(C, ROWS, c)
    mc.sort_case(emul_lib, emul_ctx, C, ROWS, mc.SETS, bases=h, c=c, rows=ROWS, mont=(0, 1) if c == 17 else (0,), one_pass=False)


@pytest.mark.parametrize("stride", [2, 3])
def test_sort_strided_tables(emul_lib, emul_ctx, bases, stride):
    """Tables for every second / third window at c = 8 (32 windows; 3 does not divide them): window w lands in bucket set
    w % stride and reads table block w / stride."""
    h = bases.get(BLS12_381, ROWS, 8, stride)
    mc.sort_case(emul_lib, emul_ctx, BLS12_381, ROWS, mc.SETS, bases=h, c=8, stride=stride, rows=ROWS, one_pass=False)
    # fewer scalars than the handle has rows: the values keep the handle's row stride
    mc.sort_case(emul_lib, emul_ctx, BLS12_381, 333, ("uniform", "edges"), bases=h, c=8, stride=stride, rows=ROWS, one_pass=False)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_sort_one_pass(emul_lib, emul_ctx, bases, C):
    """2^17 buckets (c = 17, stride 2: 512 first-level bins against the 256 of the emulator build): msm_digits_kernel,
    the split scan and msm_scatter_kernel with wave_agg_inc.  The periodic sets put exactly m key groups per window into a wave:
    up to three are served by the leader rounds alone, four and five leave lanes for the individual atomics."""
    h = bases.get(C, ROWS, 17, 2)
    mc.sort_case(emul_lib, emul_ctx, C, ROWS, mc.SETS, bases=h, c=17, stride=2, rows=ROWS, mont=(0, 1) if C is BN254 else (0,),
                 one_pass=True)
    mc.sort_case(emul_lib, emul_ctx, C, 65, ("uniform", "periodic-5", "edges"), bases=h, c=17, stride=2, rows=ROWS, one_pass=True)


def test_sort_diagnostic_arguments(emul_lib, emul_ctx, bases):
    mc.argument_checks(emul_lib, emul_ctx, BLS12_381)
    from snark_amd._binding import Ark355Error, EINVAL
    h = bases.get(BLS12_381, ROWS, 8)
    ks = mc.scalar_set("uniform", BLS12_381.r, 8, 32, ROWS + 1)
    with pytest.raises(Ark355Error) as e:         # more scalars than the handle has rows
        emul_lib.diag_msm_sort(emul_ctx, BLS12_381.curve_id, mc.scalar_bytes(BLS12_381, ks, 0), ROWS + 1, bases=h, arrays=False)
    assert e.value.code == EINVAL
    with pytest.raises(Ark355Error) as e:         # a handle of the other curve
        emul_lib.diag_msm_sort(emul_ctx, BN254.curve_id, mc.scalar_bytes(BN254, ks[:5], 0), 5, bases=h, arrays=False)
    assert e.value.code == EINVAL


def test_one_pass_sort_end_to_end(emul_lib, emul_ctx, emul_policy):
    """The one-pass sort feeding accumulation and tails: scalars around the negation threshold over resident bases with known
    discrete logs, two bucket sets of 2^16."""
    emul_policy.setenv("ARK355_MSM_C", "17")
    emul_policy.setenv("ARK355_TABLE_STRIDE", "2")
    pc.resident_known_dlog_case(emul_lib, emul_ctx, BLS12_381, 1, ROWS, _to_dev)


@pytest.mark.parametrize("name", ["equal", "periodic-4", "edges"])
def test_skewed_sets_end_to_end(emul_lib, emul_ctx, emul_policy, name):
    """Equal and periodic scalars through accumulation and tails at c = 13 with 16 entries per lane: every window has one / four
    buckets of hundreds of entries -- more heavy buckets than the heavy merge has workgroups (3 in this build, each heavy from
    three segments on), so every workgroup loops over its share of the list -- and the edge set end to end."""
    emul_policy.setenv("ARK355_MSM_C", "13")
    emul_policy.setenv("ARK355_MSM_SEG", "16")
    C = BLS12_381
    plan = mc.expected_plan(C, 13, True, 1, ROWS)
    ks = mc.scalar_set(name, C.r, 13, plan["windows"], ROWS)
    if name != "edges":
        heavy, segs = mc.heavy_buckets(ks, C.r, plan, 16, 2)
        assert 3 < heavy <= segs // 2, (heavy, segs)
    mc.known_dlog_case(emul_lib, emul_ctx, C, 1, ks, _to_dev)


@pytest.mark.parametrize("sched", ["0", "1"])
def test_prove_with_mixed_windows(emul_lib, emul_ctx, emul_policy, sched):
    """Policy MSM_C_H: the h_query table on another window size (8) than the four other tables (5, which negates high scalars).
    The four G1 tails then cannot share launches: a one-stream proof falls back to one reduction per MSM, each with its own
    part count.  Proof bytes == oracle on one stream and on the pipeline."""
    emul_policy.setenv("ARK355_SCHED", sched)
    emul_policy.setenv("ARK355_MSM_C", "5")
    emul_policy.setenv("ARK355_MSM_C_H", "8")
    C = BLS12_381
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 1030)
    pc.prove_case(emul_lib, emul_ctx, C, A, B, Cm, z, ell, rs=((5, 7),))
