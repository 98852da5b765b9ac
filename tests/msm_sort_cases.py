"""The sort stage of the MSMs (snark_amd/csrc/msm_impl.cuh: signed window digits, bucket histogram, exclusive scan, placement)
against a reference in plain Python integers, through ark355_diag_msm_sort -- shared by the CPU-emulator tier
(tests/test_emul_msm_sort.py) and the GPU tier (tests/test_gpu_msm_sort.py).

The reference knows nothing of the library: window counts and the negation of high scalars follow from the window size and the
scalar width, the digits from shifts and masks on Python integers, and every scalar it decodes is recomposed and compared with
itself before its digits are used."""
from __future__ import annotations

import random

import numpy as np

from oracle import serialize as Z
from oracle.curves import g1, g2

SETS = ("uniform", "equal", "boolean", "periodic-2", "periodic-3", "periodic-4", "periodic-5", "zero", "edges")
BASIC_SETS = ("uniform", "equal", "edges")


# ---- the plan, from the window size and the scalar width alone ---------------------------------------------------------
def oneshot_window(n, bits):
    """Window size of an MSM without tables: ceil(log2 n) - 4 clamped to [4, 16], then the nearest size (larger first) whose top
    window still holds min(c, 7) of the bits + 1 carry bit."""
    lg = 0
    while (1 << lg) < max(n, 1):
        lg += 1
    target = min(max(lg - 4, 4), 16)

    def top_bits(c):
        return bits + 1 - (-(-(bits + 1) // c) - 1) * c
    for d in range(17):
        for cand in (target + d, target - d):
            if 4 <= cand <= 16 and top_bits(cand) >= min(cand, 7):
                return cand
    raise AssertionError("no window size")


def expected_plan(C, c, resident, stride=1, rows=0):
    bits = C.r.bit_length()
    windows = -(-(bits + 1) // c)                    # one more bit than the scalar: the top window never carries out
    negate = 0
    if resident and -(-bits // c) < windows:         # r - k for k above (r - 1) / 2 is a bit shorter: a whole window less
        negate, windows = 1, -(-bits // c)
    wstride = min(stride, windows) if resident else windows
    return {"c": c, "windows": windows, "wstride": wstride, "key_windows": wstride, "total_buckets": wstride << (c - 1),
            "negate_high": negate, "row_stride": rows if resident else 0}


# ---- the reference digits ------------------------------------------------------------------------------------------------
def signed_digits(k, c, windows):
    """k = sum_w (-1)^neg_w d_w 2^(c w) with every d_w in [0, 2^(c-1)]: a raw digit above 2^(c-1) becomes 2^c - digit, negative,
    and carries one into the next window; exactly 2^(c-1) stays positive."""
    half, full = 1 << (c - 1), 1 << c
    ds, negs, carry = [], [], 0
    for w in range(windows):
        d = ((k >> (c * w)) & (full - 1)) + carry
        if d > half:
            d, neg, carry = full - d, 1, 1
        else:
            neg, carry = 0, 0
        assert 0 <= d <= half
        ds.append(d)
        negs.append(neg)
    assert carry == 0 and (k >> (c * windows)) == 0, "the top window carried out"
    return ds, negs


def scalar_digits(k, r, c, windows, negate_high):
    """Digits and signs of scalar k under the plan, self-checked: they recompose to k modulo r."""
    assert 0 <= k < r
    flip = 0
    v = k
    if negate_high and k > (r - 1) // 2:
        v, flip = r - k, 1
    ds, negs = signed_digits(v, c, windows)
    negs = [s ^ flip for s in negs]
    assert sum((-d if s else d) << (c * w) for w, (d, s) in enumerate(zip(ds, negs))) % r == k
    return ds, negs


def expected_entries(ks, r, plan):
    """(keys, vals) of every non-zero digit, in scalar-major order (the library's order is unspecified)."""
    c, windows, ws, rows = plan["c"], plan["windows"], plan["wstride"], plan["row_stride"]
    n = len(ks)
    cache = {}
    D = np.zeros((n, windows), dtype=np.int64)
    S = np.zeros((n, windows), dtype=np.int64)
    for i, k in enumerate(ks):
        t = cache.get(k)
        if t is None:
            t = cache[k] = scalar_digits(k, r, c, windows, plan["negate_high"])
        D[i], S[i] = t
    w = np.arange(windows, dtype=np.int64)[None, :]
    i = np.arange(n, dtype=np.int64)[:, None]
    keys = (w % ws) * (1 << (c - 1)) + D - 1
    vals = ((w // ws) * rows + i) | (S << 31)
    m = D != 0
    return keys[m].astype(np.uint32), vals[m].astype(np.uint32)


# ---- scalar sets -----------------------------------------------------------------------------------------------------------
def edge_scalars(r, c, windows):
    half = (r - 1) // 2
    B, F = 1 << (c - 1), 1 << c
    xs = [0, 1, 2, r - 1, r - 2, half, half - 1, half + 1,
          B, B - 1, B + 1, F - 1, F, F + 1]
    for w in sorted({1, 2, 3, windows // 2, windows - 2, windows - 1}):
        if w >= 1:
            xs += [(1 << (c * w)) - 1, 1 << (c * w), 1 << (c * w - 1)]
    # every digit exactly 2^(c-1) -- over all windows and over all but the top one (under negate_high only values up to
    # (r - 1) / 2 are decoded as they are) -- and their negatives, whose decoded form has every sign flipped
    for top in (windows, windows - 1):
        v = sum(B << (c * w) for w in range(top))
        xs += [v, r - v % r]
    xs += [(1 << (c * (windows - 1))) - 1, r - ((1 << (c * (windows - 1))) - 1) % r]     # a carry chain that ends in the top window
    # exactly 2^(c-1) in window 0 (positive, no carry), then a raw digit 2^c - 1 (negative one, carries) and zero digits that
    # still carry (2^c - 1 behind a carry) up to the top window
    xs.append((1 << (c * (windows - 1))) - B)
    return [x % r for x in xs]


def scalar_set(name, r, c, windows, n, seed=1):
    rnd = random.Random("%s/%d/%d/%d" % (name, c, n, seed))
    if name == "uniform":
        return [rnd.randrange(r) for _ in range(n)]
    if name == "equal":
        return [rnd.randrange(r)] * n
    if name == "boolean":
        return [rnd.randrange(2) if rnd.random() < 0.9 else rnd.randrange(r) for _ in range(n)]
    if name.startswith("periodic-"):
        m = int(name.split("-")[1])
        v = [rnd.randrange(r) for _ in range(m)]
        return [v[i % m] for i in range(n)]
    if name == "zero":
        return [0] * n
    if name == "edges":
        e = edge_scalars(r, c, windows)
        return [e[i % len(e)] for i in range(n)]
    raise KeyError(name)


def scalar_bytes(C, ks, mont):
    if mont:
        return b"".join(((k << 256) % C.r).to_bytes(32, "little") for k in ks)
    return b"".join(k.to_bytes(32, "little") for k in ks)


# ---- the comparison ----------------------------------------------------------------------------------------------------------
def compare(got, ks, r, plan, what):
    for name, v in plan.items():
        assert got[name] == v, (what, name, got[name], v)
    keys, vals = expected_entries(ks, r, plan)
    nb = plan["total_buckets"]
    hist = np.bincount(keys, minlength=nb).astype(np.uint32)
    assert got["total"] == len(keys), (what, got["total"], len(keys))
    bad = np.nonzero(got["counts"] != hist)[0]
    assert bad.size == 0, (what, "counts", bad[:4], got["counts"][bad[:4]], hist[bad[:4]])
    excl = np.zeros(nb, dtype=np.uint64)
    np.cumsum(hist[:-1], out=excl[1:])
    bad = np.nonzero(got["offsets"] != excl)[0]
    assert bad.size == 0, (what, "offsets", bad[:4], got["offsets"][bad[:4]], excl[bad[:4]])
    sk, sv = got["sorted_keys"], got["sorted_vals"]
    assert sk.shape == keys.shape and sv.shape == vals.shape, (what, sk.shape, keys.shape)
    assert np.all(sk[1:] >= sk[:-1]), (what, "sorted_keys decrease")
    assert np.array_equal(sk, np.sort(keys)), (what, "sorted_keys")
    ge, gg = np.lexsort((vals, keys)), np.lexsort((sv, sk))
    assert np.array_equal(sk[gg], keys[ge]) and np.array_equal(sv[gg], vals[ge]), (what, "(key, value) pairs")


def sort_case(lib, ctx, C, n, names, bases=None, c=None, stride=1, rows=0, mont=(0,), one_pass=None, seed=1):
    """The sort diagnostic over the scalar sets `names`, each tiled to n.  bases=None: the one-shot plan (window size from
    oneshot_window); a handle: loaded under MSM_C=c / TABLE_STRIDE=stride with `rows` rows.  one_pass: the sort the shape must reach."""
    resident = bases is not None
    if not resident:
        c = oneshot_window(n, C.r.bit_length())
    plan = expected_plan(C, c, resident, stride, rows)
    for name in names:
        ks = scalar_set(name, C.r, c, plan["windows"], n, seed)
        for m in mont:
            what = (C.name, "resident" if resident else "one-shot", c, stride, n, name, "mont" if m else "canonical")
            got = lib.diag_msm_sort(ctx, C.curve_id, scalar_bytes(C, ks, m), n, mont=m, bases=bases)
            if one_pass is not None:
                assert got["one_pass"] == int(one_pass), (what, got["one_pass"])
            compare(got, ks, C.r, plan, what)


class BasesCache:
    """ark355_bases handles keyed by (curve, group, rows, c, stride): the sort reads only the plan of a handle, so every scalar
    set of a shape shares one table build.  The points are copies of the generator (no accumulation runs over them)."""

    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.h = lib, ctx, {}

    def get(self, C, rows, c, stride=1):
        key = (C.name, rows, c, stride)
        if key not in self.h:
            with self.lib.policy(self.ctx, MSM_C=c, TABLE_STRIDE=stride):
                self.h[key] = self.lib.bases_load(self.ctx, C.curve_id, 1, Z.g1_raw(C, g1(C).gen) * rows, rows)
        return self.h[key]

    def close(self):
        for h in self.h.values():
            self.lib.dll.ark355_bases_free(h)
        self.h = {}


def argument_checks(lib, ctx, C):
    """Capacities below what the plan needs are refused, after the plan and the total were written; n = 0 sorts nothing."""
    import ctypes as Ct
    from snark_amd._binding import EINVAL, SORT_PLAN_WORDS
    n = 65
    ks = scalar_set("uniform", C.r, 4, 64, n)
    sb = np.frombuffer(scalar_bytes(C, ks, 0), dtype=np.uint8)
    head = lib.diag_msm_sort(ctx, C.curve_id, sb, n, arrays=False)
    nb, ne = head["total_buckets"], head["total"]
    plan, total = (Ct.c_uint32 * SORT_PLAN_WORDS)(), Ct.c_uint32(0)
    a, b = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32)
    k, v = np.full(ne, 7, dtype=np.uint32), np.full(ne, 7, dtype=np.uint32)
    call = lib.dll.ark355_diag_msm_sort
    p = sb.ctypes.data
    assert call(ctx, C.curve_id, None, p, n, 0, Ct.byref(plan), a.ctypes.data, b.ctypes.data, nb - 1, None, None, 0, Ct.byref(total)) == EINVAL
    assert plan[4] == nb and total.value == ne
    assert call(ctx, C.curve_id, None, p, n, 0, Ct.byref(plan), None, None, 0, k.ctypes.data, v.ctypes.data, ne - 1, Ct.byref(total)) == EINVAL
    assert np.all(k == 7) and np.all(v == 7)                 # nothing was copied into the short arrays
    assert call(ctx, C.curve_id, None, p, n, 0, Ct.byref(plan), a.ctypes.data, None, nb, None, None, 0, Ct.byref(total)) == EINVAL
    assert call(ctx, 99, None, p, n, 0, Ct.byref(plan), None, None, 0, None, None, 0, Ct.byref(total)) == EINVAL
    assert call(ctx, C.curve_id, None, None, n, 0, Ct.byref(plan), None, None, 0, None, None, 0, Ct.byref(total)) == EINVAL
    assert call(ctx, C.curve_id, None, p, n, 0, None, None, None, 0, None, None, 0, Ct.byref(total)) == EINVAL
    assert call(ctx, C.curve_id, None, p, n, 0, Ct.byref(plan), None, None, 0, None, None, 0, None) == EINVAL
    got = lib.diag_msm_sort(ctx, C.curve_id, b"", 0)
    assert got["total"] == 0 and not got["counts"].any() and not got["offsets"].any() and got["sorted_keys"].size == 0


# ---- end to end over chosen scalars: bases with known discrete logs ----------------------------------------------------------
def known_dlog_case(lib, ctx, C, group, ks, to_dev=None, seed=33):
    """sum k_i (s_i G) == (sum k_i s_i) G for the given scalars: over resident bases (to_dev places the scalars in device memory;
    the handle is loaded under the context's current MSM_C / TABLE_STRIDE) or, with to_dev=None, as a one-shot ark355_msm_g1 / _g2."""
    n = len(ks)
    rnd = random.Random(seed + n)
    G_ = g1(C) if group == 1 else g2(C)
    raw = Z.g1_raw if group == 1 else Z.g2_raw
    fromraw = Z.g1_from_raw if group == 1 else Z.g2_from_raw
    sz = lib.sizes(C.curve_id)
    psz = sz["g1"] if group == 1 else sz["g2"]
    ss = [rnd.getrandbits(64) + 1 for _ in range(n)]
    bases = lib.fixed_base_mul(ctx, C.curve_id, group, raw(C, G_.gen), b"".join(Z.fr_canon(C, s) for s in ss), n, psz)
    expect = G_.mul(G_.gen, sum(k * s for k, s in zip(ks, ss)) % C.r)
    sb = scalar_bytes(C, ks, 0)
    if to_dev is None:
        out = lib.msm(ctx, C.curve_id, group, bases, sb, n, psz)
    else:
        h = lib.bases_load(ctx, C.curve_id, group, bases, n)
        try:
            ptr, keep = to_dev(sb)
            out = lib.msm_dev(ctx, h, ptr, n, 0, psz)
        finally:
            lib.dll.ark355_bases_free(h)
    assert fromraw(C, out) == expect, (C.name, group, n)


def heavy_buckets(ks, r, plan, seg_len, min_span):
    """From the reference digits alone: (buckets the merge hands to the heavy kernel, segments).  The sorted entries are cut into
    segments of seg_len; a bucket is heavy when its entries reach over more than max(min_span, twice the average span) segment
    boundaries."""
    keys, _ = expected_entries(ks, r, plan)
    cnt = np.bincount(keys, minlength=plan["total_buckets"]).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(cnt)[:-1]))
    segs = -(-plan["windows"] * len(ks) // seg_len)
    span = max(min_span, 2 * (-(-segs // plan["total_buckets"])))
    m = cnt > 0
    heavy = int(np.count_nonzero((off[m] + cnt[m] - 1) // seg_len - off[m] // seg_len > span))
    return heavy, segs
