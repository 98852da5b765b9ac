"""GPU tier (-m gpu): the sort stage of the MSMs on the device, through ark355_diag_msm_sort, against the plain-integer reference
of tests/msm_sort_cases.py -- and the paths behind it that no other test reaches: the one-pass counting sort above 2^20 buckets
(msm_digits_kernel / msm_scatter_kernel with the wave-aggregated atomics of wave_agg_inc), the split scan from its first shape
to two tiles per span, a heavy-bucket list longer than the heavy merge's grid, and keys whose h_query table has a window size of
its own.  Every shape is the smallest at which its path exists.  CPU twin: tests/test_emul_msm_sort.py."""
import random

import numpy as np
import pytest

import msm_sort_cases as mc
import parity_cases as pc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
ROWS = 1100            # resident shapes: the policy's window size applies from 1024 rows on


def _to_dev(b):
    import torch
    t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.fixture(scope="module")
def bases(gpu_lib, gpu_ctx):
    cache = mc.BasesCache(gpu_lib, gpu_ctx)
    yield cache
    cache.close()


def _one_pass(c, stride):
    return (stride << (c - 1)) > (1 << 20)          # more than 4096 first-level bins of 256 buckets


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 8197, 1 << 15])
@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_sort_one_shot(gpu_lib, gpu_ctx, C, n):
    """The plan without tables: partial waves, the 4096-scalar workgroup of the first sort level from one short of it to one
    past two of them, and 2^15 scalars at c = 13 with 20 bucket sets."""
    if C is BN254 and n not in (65, 4097, 1 << 15):
        n_sets = ("edges",)
    else:
        n_sets = mc.BASIC_SETS
    mc.sort_case(gpu_lib, gpu_ctx, C, n, n_sets, mont=(0, 1) if n in (65, 4097) else (0,), one_pass=False)


# (curve, scalars, window, stride, scalar sets).  Buckets = stride x 2^(c-1): 2^16 is the last single-workgroup scan, 2^17 the
# first split scan (8 spans), 2^19 32 spans and a 4096-entry second-level tile over hundreds of bins, 2^21 and 3 x 2^19 the
# one-pass sort, 2^23 the one-pass sort with 512 scan tiles in 256 spans of two.
_BIG = (1 << 16) + 77
RESIDENT = (
    [(BLS12_381, ROWS, c, 1, mc.SETS if _one_pass(c, 1) else mc.BASIC_SETS) for c in (13, 16, 17, 18, 20, 22, 24)]
    + [(BLS12_381, 8197, 17, 1, mc.BASIC_SETS), (BLS12_381, 8197, 20, 1, mc.BASIC_SETS)]
    + [(BLS12_381, _BIG, 17, 1, (s,)) for s in mc.BASIC_SETS]
    + [(BLS12_381, _BIG, 22, 1, (s,)) for s in mc.SETS]
    + [(BLS12_381, ROWS, 13, 2, mc.BASIC_SETS), (BLS12_381, ROWS, 13, 3, mc.BASIC_SETS), (BLS12_381, ROWS, 20, 3, mc.SETS)]
    + [(BN254, ROWS, 16, 1, mc.BASIC_SETS), (BN254, ROWS, 17, 1, mc.BASIC_SETS)]
)


@pytest.mark.parametrize("C,n,c,stride,sets", RESIDENT,
                         ids=["%s-n%d-c%d-s%d-%s" % (C.name, n, c, s, sets[0] if len(sets) == 1 else len(sets)) for C, n, c, s, sets in RESIDENT])
def test_sort_resident(gpu_lib, gpu_ctx, bases, C, n, c, stride, sets):
    h = bases.get(C, n, c, stride)
    mont = (0, 1) if (n == ROWS and c in (17, 22)) or (n == _BIG and sets[0] == "edges") else (0,)
    mc.sort_case(gpu_lib, gpu_ctx, C, n, sets, bases=h, c=c, stride=stride, rows=n, mont=mont, one_pass=_one_pass(c, stride))


def test_sort_fewer_scalars_than_rows(gpu_lib, gpu_ctx, bases):
    """A prefix of a handle's rows on the one-pass path: the values keep the handle's row stride."""
    h = bases.get(BLS12_381, ROWS, 22, 1)
    mc.sort_case(gpu_lib, gpu_ctx, BLS12_381, 257, ("uniform", "periodic-5", "edges"), bases=h, c=22, rows=ROWS, one_pass=True)


def test_sort_diagnostic_arguments(gpu_lib, gpu_ctx):
    mc.argument_checks(gpu_lib, gpu_ctx, BLS12_381)


# ---- end to end: the same paths through accumulation and tails ------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_one_pass_sort_end_to_end(gpu_lib, gpu_ctx, gpu_policy, group):
    """MSM_C = 22: 2^21 bucket slots through the one-pass sort, the merge and the row / column / bit sums, scalars around the
    negation threshold, against the known discrete log."""
    gpu_policy.setenv("ARK355_MSM_C", "22")
    pc.resident_known_dlog_case(gpu_lib, gpu_ctx, BLS12_381, group, ROWS, _to_dev)


@pytest.mark.parametrize("name", ["equal", "periodic-4"])
def test_one_pass_sort_end_to_end_skewed(gpu_lib, gpu_ctx, gpu_policy, name):
    gpu_policy.setenv("ARK355_MSM_C", "22")
    C = BLS12_381
    plan = mc.expected_plan(C, 22, True, 1, ROWS)
    mc.known_dlog_case(gpu_lib, gpu_ctx, C, 1, mc.scalar_set(name, C.r, 22, plan["windows"], ROWS), _to_dev)


def test_one_pass_sort_end_to_end_strided(gpu_lib, gpu_ctx, gpu_policy):
    """MSM_C = 20 with tables for every third window: three bucket sets of 2^19, 6144 first-level bins."""
    gpu_policy.setenv("ARK355_MSM_C", "20")
    gpu_policy.setenv("ARK355_TABLE_STRIDE", "3")
    pc.resident_known_dlog_case(gpu_lib, gpu_ctx, BLS12_381, 1, ROWS, _to_dev)


@pytest.mark.parametrize("C,group", [(BLS12_381, 1), (BN254, 1), (BLS12_381, 2)], ids=lambda v: getattr(v, "name", str(v)))
def test_heavy_list_longer_than_the_heavy_grid(gpu_lib, gpu_ctx, gpu_policy, C, group):
    """A one-shot MSM of 2^15 terms whose scalars are drawn from 16 values, 16 entries per lane: every window has up to 16 buckets
    of ~2048 entries, each over ~128 segments -- heavy from 48 on -- so the heavy list (320 buckets by the reference digits) is
    longer than the 128 workgroups of msm_merge_heavy28_kernel and each of them takes a second and third bucket."""
    gpu_policy.setenv("ARK355_MSM_SEG", "16")
    n = 1 << 15
    rnd = random.Random(355)
    pool = [rnd.randrange(C.r) for _ in range(16)]
    ks = [pool[rnd.randrange(16)] for _ in range(n)]
    c = mc.oneshot_window(n, C.r.bit_length())
    assert c == 13
    heavy, segs = mc.heavy_buckets(ks, C.r, mc.expected_plan(C, c, False), 16, 48)
    print("heavy buckets %d, segments %d, list capacity %d" % (heavy, segs, segs // 48 + 1))
    assert 128 < heavy <= segs // 48, (heavy, segs)
    mc.known_dlog_case(gpu_lib, gpu_ctx, C, group, ks)


@pytest.mark.parametrize("sched", ["0", "1"])
@pytest.mark.parametrize("c,c_h", [(13, 17), (16, 13)])
def test_prove_with_mixed_windows(gpu_lib, gpu_ctx, gpu_policy, c, c_h, sched):
    """Policy MSM_C_H: the h_query table on a window size of its own -- 17 against 13, where H alone negates the scalars above
    (r - 1) / 2, and 13 against 16.  The four G1 tails of a one-stream proof cannot share launches then and run per MSM, each
    with its own part count.  Proof bytes == oracle on one stream and on the pipeline."""
    gpu_policy.setenv("ARK355_SCHED", sched)
    gpu_policy.setenv("ARK355_MSM_C", str(c))
    gpu_policy.setenv("ARK355_MSM_C_H", str(c_h))
    C = BLS12_381
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 1030)
    pc.prove_case(gpu_lib, gpu_ctx, C, A, B, Cm, z, ell, rs=((C.r - 3, 12345),))
