"""The MSM tail kernels (snark_amd/csrc/tails28_impl.cuh: merge, heavy merge, row / column sums, bit sums) and the host's Horner
driven through doublings, cancellations and empties -- shared by the CPU-emulator tier (tests/test_emul_msm_tails.py) and the GPU
tier (tests/test_gpu_msm_tails.py).

Sums of random points never meet equal, opposite or empty operands in the tails' own general addition (add28 / add28_g2 and their
cold paths).  Here every base is a small multiple m_i P of one point P = s G, so what a bucket, a row, a column or a partial run
holds is a small integer multiple of P that the test computes first: the integer bucket matrix

    M[set][b] = sum of +-m_i 2^(c wstride (w // wstride)) over the entries of bucket b          (in units of P, modulo r)

follows from the plain-integer reference digits of tests/msm_sort_cases.py, each design asserts ON INTEGERS that M has the property
it is named for (these properties hold for any dealing of items to lanes), and only then is the library called.  The expected point
is (sum k_i m_i s mod r) G by the oracle's group law."""
from __future__ import annotations

import random

import numpy as np

import msm_sort_cases as mc
from oracle import serialize as Z
from oracle.curves import g1, g2

SEG = 16                                     # MSM_SEG of the merge designs: entries per accumulation lane
FUZZ_SEEDS = (1, 2, 3)
MATRIX_DESIGNS = (("constant", "alternating", "halves", "single-first", "single-last", "single-middle", "zero")
                  + tuple("fuzz-%d" % s for s in FUZZ_SEEDS))
ONESHOT_DESIGNS = ("constant", "alternating") + tuple("fuzz-%d" % s for s in FUZZ_SEEDS)


def split(c):
    """(lb, hb): the low bits of a bucket index are its column, the high bits its row (tails28_split)."""
    lb = c // 2
    return lb, c - 1 - lb


def centred(v, r):
    v %= r
    return v if v <= r // 2 else v - r


# ---- the tier: library, context, how scalars reach "device" memory, the heavy threshold of the build --------------------------
class Tier:
    def __init__(self, lib, ctx, to_dev, min_span):
        self.lib, self.ctx, self.to_dev, self.min_span = lib, ctx, to_dev, min_span
        self._pts = {}

    def group(self, C, group):
        G_ = g1(C) if group == 1 else g2(C)
        sz = self.lib.sizes(C.curve_id)
        return G_, (Z.g1_raw if group == 1 else Z.g2_raw), (Z.g1_from_raw if group == 1 else Z.g2_from_raw), sz["g1"] if group == 1 else sz["g2"]

    def dlog(self, C, group):
        """s of P = s G: one seeded value per curve and group."""
        return random.Random("tails/%s/%d" % (C.name, group)).randrange(2, C.r)

    def point(self, C, group, m):
        """Raw bytes of m P, made by ark355_fixed_base_mul and checked against the oracle's scalar multiplication; m = 0: infinity."""
        key = (C.name, group, m)
        if key not in self._pts:
            G_, raw, fromraw, psz = self.group(C, group)
            k = m * self.dlog(C, group) % C.r
            b = self.lib.fixed_base_mul(self.ctx, C.curve_id, group, raw(C, G_.gen), Z.fr_canon(C, k), 1, psz)
            assert fromraw(C, b) == G_.mul(G_.gen, k), (C.name, group, m)
            assert (b == bytes(psz)) == (m == 0)
            self._pts[key] = b
        return self._pts[key]

    def bases(self, C, group, ms):
        return b"".join(self.point(C, group, m) for m in ms)

    def expect(self, C, group, ks, ms):
        G_ = self.group(C, group)[0]
        return G_.mul(G_.gen, sum(k * m for k, m in zip(ks, ms)) * self.dlog(C, group) % C.r)

    def resident(self, C, group, ks, ms, mont=0):
        """ark355_bases_load + ark355_msm_dev under the context's current policy; the affine result (None: infinity)."""
        _, _, fromraw, psz = self.group(C, group)
        n = len(ks)
        h = self.lib.bases_load(self.ctx, C.curve_id, group, self.bases(C, group, ms), n)
        try:
            ptr, keep = self.to_dev(mc.scalar_bytes(C, ks, mont))
            return fromraw(C, self.lib.msm_dev(self.ctx, h, ptr, n, mont, psz))
        finally:
            self.lib.dll.ark355_bases_free(h)

    def oneshot(self, C, group, ks, ms):
        _, _, fromraw, psz = self.group(C, group)
        return fromraw(C, self.lib.msm(self.ctx, C.curve_id, group, self.bases(C, group, ms), mc.scalar_bytes(C, ks, 0), len(ks), psz))


# ---- the reference: integer bucket matrix and the sums the tails form from it ----------------------------------------------------
def bucket_matrix(ks, ms, r, plan):
    """M[set][b] in units of P, centred modulo r, from the reference digits; checked against sum k_i m_i with the weights of
    msm_finish_host (bucket b counts b + 1 times, set j 2^(c j) times)."""
    c, ws, rows, B = plan["c"], plan["wstride"], plan["row_stride"], 1 << (plan["c"] - 1)
    keys, vals = mc.expected_entries(ks, r, plan)
    flat = [0] * plan["total_buckets"]
    for key, val in zip(keys.tolist(), vals.tolist()):
        q, i = divmod(val & 0x7FFFFFFF, rows) if rows else (0, val & 0x7FFFFFFF)
        t = ms[i] << (c * ws * q)
        flat[key] += -t if val >> 31 else t
    M = [[centred(v, r) for v in flat[j * B:(j + 1) * B]] for j in range(plan["key_windows"])]
    total = sum(sum((b + 1) * v for b, v in enumerate(row)) << (c * j) for j, row in enumerate(M))
    assert (total - sum(k * m for k, m in zip(ks, ms))) % r == 0, "the reference matrix does not recompose to sum k_i m_i"
    return M


def tail_sums(Mset, c):
    """Row sums D_hi, column sums C_lo and the c bit sums of one bucket set, as integers; the bit sums recompose to
    sum (b + 1) M_b the way msm_finish_host combines them."""
    lb, hb = split(c)
    L, H = 1 << lb, 1 << hb
    assert len(Mset) == L * H
    D = [sum(Mset[hi * L:(hi + 1) * L]) for hi in range(H)]
    Cs = [sum(Mset[lo::L]) for lo in range(L)]
    p = [sum(Cs[i] for i in range(L) if i >> k & 1) for k in range(lb)]
    p += [sum(D[i] for i in range(H) if i >> k & 1) for k in range(hb)]
    p.append(sum(D[i] for i in range(H) if not i >> (hb - 1) & 1))
    assert len(p) == c
    assert sum(v << k for k, v in enumerate(p[:c - 1])) + p[c - 2] + p[c - 1] == sum((b + 1) * v for b, v in enumerate(Mset))
    return D, Cs, p


def multipliers(design, B):
    """m_b of every bucket of one set."""
    if design == "constant":
        return [1] * B
    if design == "alternating":
        return [-1 if b & 1 else 1 for b in range(B)]
    if design == "halves":
        return [1 if b < B // 2 else -1 for b in range(B)]
    if design.startswith("single-"):
        at = {"first": 0, "last": B - 1, "middle": B // 2 + B // 8 + 3}[design.split("-")[1]]
        return [1 if b == at else 0 for b in range(B)]
    if design == "zero":
        return [0] * B
    if design.startswith("fuzz-"):
        rnd = random.Random("tail-fuzz/%s/%d" % (design, B))
        return [rnd.randrange(-2, 3) for _ in range(B)]
    raise KeyError(design)


def assert_design(design, Mset, c):
    """The property a design is named for, on the integer matrix of one whole bucket set (B = 2^(c-1) buckets)."""
    lb, hb = split(c)
    L, H, B = 1 << lb, 1 << hb, 1 << (c - 1)
    D, Cs, p = tail_sums(Mset, c)
    assert Mset == multipliers(design, B), (design, c)
    if design == "constant":
        # any two partial sums over equally many buckets are equal and not infinity: every addition of two of them doubles
        assert set(Mset) == {1} and set(D) == {L} and set(Cs) == {H}
        assert sum((b + 1) * v for b, v in enumerate(Mset)) == B * (B + 1) // 2
    elif design == "alternating":
        # neighbours cancel: every row sum is infinity, the column sums are +-H P; equal-parity partial sums are equal
        assert all(Mset[b] == -Mset[b + 1] for b in range(0, B, 2))
        assert set(D) == {0} and Cs == [-H if lo & 1 else H for lo in range(L)]
        assert p[lb:] == [0] * (hb + 1) and p[0] == -H * (L // 2)
    elif design == "halves":
        # every column sum is infinity; the top-bit sum of the rows and its complement are -+(H/2) L P and cancel on the host
        assert set(Cs) == {0} and D == [L if hi < H // 2 else -L for hi in range(H)]
        assert p[:lb] == [0] * lb and p[c - 2] == -(H // 2) * L and p[c - 1] == (H // 2) * L and p[c - 2] + p[c - 1] == 0
    elif design.startswith("single-"):
        assert sorted(Mset)[-2:] == [0, 1] and sum(Mset) == 1              # one bucket; every other operand is empty
        assert sum(1 for v in D if v) == 1 and sum(1 for v in Cs if v) == 1
    elif design == "zero":
        assert not any(Mset) and not any(p)
    elif design.startswith("fuzz-"):
        # equal, opposite and empty operands among the buckets of a row and among the row / column sums (8 buckets, the one-shot
        # shape: among the buckets)
        assert any(sum(x) != 0 for x in (D, Cs)) and sum((b + 1) * v for b, v in enumerate(Mset)) != 0
        pairs = [(Mset[i], Mset[j]) for i in range(min(B, L)) for j in range(i)]
        assert any(a == b != 0 for a, b in pairs) or any(a == -b != 0 for a, b in pairs)
        if B >= 1024:
            assert set(Mset) == {-2, -1, 0, 1, 2}
            row = Mset[:L]
            assert any(row[i] == row[i + 1] != 0 for i in range(L - 1)) and any(row[i] == -row[i + 1] != 0 for i in range(L - 1))
            both = D + Cs
            assert 0 in both and len(set(both)) < len(both) and any(-v in both for v in both if v)
    else:
        raise KeyError(design)


def nontrivial(design, total, r):
    if design == "zero":
        assert total % r == 0
    else:
        assert total % r != 0, (design, "the expected point is infinity")


# ---- bucket-matrix designs over resident bases: one entry per bucket in window 0 ---------------------------------------------
def matrix_case(tier, policy, C, group, c, design, mont=0, pack=None):
    """One entry per non-empty bucket of window 0 -- scalar b + 1 (b + 1 = 2^(c-1) included: it stays positive), base m_b P --
    and a zero scalar for every empty one, which also pads to the 1024-row floor of MSM_C."""
    B = 1 << (c - 1)
    assert B >= 1024
    m = multipliers(design, B)
    ks = [b + 1 if m[b] else 0 for b in range(B)]
    ms = [m[b] if m[b] else 1 for b in range(B)]
    plan = mc.expected_plan(C, c, True, 1, B)
    M = bucket_matrix(ks, ms, C.r, plan)
    assert len(M) == 1
    assert_design(design, M[0], c)
    nontrivial(design, sum(k * v for k, v in zip(ks, ms)), C.r)
    policy.setenv("ARK355_MSM_C", str(c))
    policy.setenv("ARK355_TABLE_STRIDE", "1")
    if pack is not None:
        policy.setenv("ARK355_PACK_ROWS", str(pack))
    got = tier.resident(C, group, ks, ms, mont)
    assert got == tier.expect(C, group, ks, ms), (C.name, group, c, design, tail_sums(M[0], c)[2])


def strided_case(tier, policy, C, group, c):
    """TABLE_STRIDE = 2: window 0 fills bucket set 0 with `constant`, window 1 set 1 with `alternating`.  Scalars d + d' 2^c:
    an even bucket of set 1 shares its entry with the same bucket of set 0 (d = d'); an odd one, whose base is -P, has its own."""
    B = 1 << (c - 1)
    ks, ms = [], []
    for b in range(B):
        if b & 1:
            ks += [b + 1, (b + 1) << c]
            ms += [1, -1]
        else:
            ks.append((b + 1) + ((b + 1) << c))
            ms.append(1)
    plan = mc.expected_plan(C, c, True, 2, len(ks))
    assert plan["key_windows"] == 2
    M = bucket_matrix(ks, ms, C.r, plan)
    assert_design("constant", M[0], c)
    assert_design("alternating", M[1], c)
    nontrivial("strided", sum(k * v for k, v in zip(ks, ms)), C.r)
    policy.setenv("ARK355_MSM_C", str(c))
    policy.setenv("ARK355_TABLE_STRIDE", "2")
    assert tier.resident(C, group, ks, ms) == tier.expect(C, group, ks, ms), (C.name, group, c)


# ---- the one-shot plan at c = 4: every window below the top one holds the same design over 8 buckets -----------------------------
def oneshot_case(tier, C, group, design, dmax):
    """Entry d (1 <= d <= dmax) has digit d in every window below the top one and base m_(d-1) P: 63 bucket sets of 8 buckets with
    row / column counts 4 and 2 and stage-B counts 2 and 1 -- the shortened butterfly at its smallest -- and an empty top set.
    dmax = 7 leaves bucket 7 empty; dmax = 8 (the digit 2^(c-1), positive) fills the matrix, and the design's property holds."""
    c = mc.oneshot_window(dmax, C.r.bit_length())
    assert c == 4
    plan = mc.expected_plan(C, c, False)
    W = plan["windows"]
    m = multipliers(design, 8)
    ks, ms = [], []
    for d in range(1, dmax + 1):
        if m[d - 1]:
            ks.append(sum(d << (c * w) for w in range(W - 1)))
            ms.append(m[d - 1])
    assert 0 < len(ks) <= 256 and max(ks) < C.r
    M = bucket_matrix(ks, ms, C.r, plan)
    assert len(M) == W and not any(M[W - 1])
    for w in range(W - 1):
        assert M[w] == M[0]
        if dmax == 8:
            assert_design(design, M[w], c)
        else:
            assert M[w] == m[:7] + [0]
            tail_sums(M[w], c)
    nontrivial(design, sum(k * v for k, v in zip(ks, ms)), C.r)
    assert tier.oneshot(C, group, ks, ms) == tier.expect(C, group, ks, ms), (C.name, group, design, dmax)


# ---- merge designs: MSM_SEG = 16, resident c = 11 ----------------------------------------------------------------------------------
def merge_case(tier, policy, C, group, copies, front=0, signs=None, heavy=False, c=11):
    """`copies` entries in ONE bucket, cut into runs of 16 by the accumulation; front = 5 puts a bucket of five entries (2 P each)
    in front, so that the bucket's first run is the second of its segment and lives in tail[t0].  signs = None: every entry is
    P (all runs starting a segment are 16 P: the first merge addition, and with `heavy` every one, doubles); a seed: each entry
    P or -P; "balanced": as many of each, and the bucket -- and the MSM -- ends at infinity."""
    assert copies % SEG == 0
    if signs is None:
        sg = [1] * copies
    elif signs == "balanced":
        sg = [1, -1] * (copies // 2)
        random.Random("tail-merge/balanced/%d" % copies).shuffle(sg)
    else:
        rnd = random.Random("tail-merge/%s/%d/%d" % (signs, copies, front))
        sg = [rnd.choice((1, -1)) for _ in range(copies)]
    ks = [1] * front + [2 if front else 1] * copies
    ms = [2] * front + sg
    n = max(1024, len(ks))
    ks += [0] * (n - len(ks))
    ms += [1] * (n - len(ms))
    plan = mc.expected_plan(C, c, True, 1, n)
    # on integers: where the bucket lies in the sorted entries, what it holds, which merge kernel takes it
    keys, _ = mc.expected_entries(ks, C.r, plan)
    assert len(keys) == front + copies
    cnt = np.bincount(keys, minlength=2)
    bucket = 1 if front else 0
    assert cnt[bucket] == copies and int(cnt[:bucket].sum()) == front and (front == 0 or 0 < front < SEG)
    M = bucket_matrix(ks, ms, C.r, plan)[0]
    assert M[bucket] == sum(sg) and (not front or M[0] == 2 * front) and not any(M[2:])
    if signs is None:
        assert M[bucket] == copies                 # with front == 0 every run is the same 16 P
    if signs == "balanced":
        assert M[bucket] == 0 and sg.count(1) == sg.count(-1)
    nheavy, segs = mc.heavy_buckets(ks, C.r, plan, SEG, tier.min_span)
    assert nheavy == (1 if heavy else 0), (copies, front, nheavy, segs)
    total = sum(k * v for k, v in zip(ks, ms))
    assert (total % C.r == 0) == (signs == "balanced" and not front)
    policy.setenv("ARK355_MSM_C", str(c))
    policy.setenv("ARK355_TABLE_STRIDE", "1")
    policy.setenv("ARK355_MSM_SEG", str(SEG))
    assert tier.resident(C, group, ks, ms) == tier.expect(C, group, ks, ms), (C.name, group, copies, front, signs, M[:2])


# ---- ark355_xyzz_sum over equal, opposite and empty partials -------------------------------------------------------------------------
def xyzz_case(tier, C, group, rows=6):
    """X = sum k_i s_i G as an XYZZ partial of ark355_msm_dev_partial, -X from the same rows with the scalars r - k_i (another
    representative: the sums compare cross-multiplied coordinates), the empty partial from no rows at all."""
    G_, raw, fromraw, psz = tier.group(C, group)
    lib, ctx = tier.lib, tier.ctx
    rnd = random.Random("tail-xyzz/%s/%d" % (C.name, group))
    ss = [rnd.randrange(1, C.r) for _ in range(rows)]
    ks = [rnd.randrange(1, C.r) for _ in range(rows)]
    x = sum(k * s for k, s in zip(ks, ss)) % C.r
    assert x and 65 * x % C.r
    bases = lib.fixed_base_mul(ctx, C.curve_id, group, raw(C, G_.gen), b"".join(Z.fr_canon(C, s) for s in ss), rows, psz)
    h = lib.bases_load(ctx, C.curve_id, group, bases, rows)
    try:
        ptr, keep = tier.to_dev(mc.scalar_bytes(C, ks, 0))
        nptr, nkeep = tier.to_dev(mc.scalar_bytes(C, [C.r - k for k in ks], 0))
        X = lib.msm_dev(ctx, h, ptr, rows, 0, 2 * psz, partial=True)
        N = lib.msm_dev(ctx, h, nptr, rows, 0, 2 * psz, partial=True)
        E = lib.msm_dev(ctx, h, ptr, 0, 0, 2 * psz, partial=True)
    finally:
        lib.dll.ark355_bases_free(h)
    assert X != N and X != E

    def total(parts):
        return fromraw(C, lib.xyzz_sum(ctx, C.curve_id, group, b"".join(parts), len(parts), psz))

    def mul(k):
        return G_.mul(G_.gen, k * x % C.r)
    assert total([X]) == mul(1) and total([N]) == mul(-1) and total([E]) is None
    for name, parts, k in (("X X", [X, X], 2), ("X -X", [X, N], 0), ("X X -X empty X", [X, X, N, E, X], 2),
                           ("64 X", [X] * 64, 64), ("65 alternating", [X, N] * 32 + [X], 1)):
        assert total(parts) == mul(k), (C.name, group, name)
