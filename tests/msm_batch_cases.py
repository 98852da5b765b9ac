"""Cases of the batched short MSMs, shared by the CPU-emulator tier and the GPU tier (tests/test_emul_msm_batch.py,
tests/test_gpu_msm_batch.py): ark355_msm_batch_dev (include/ark355.h "Batched short MSMs"), the opening that hands its levels to
it, and Mle.commit_dev.  Every comparison is byte for byte.

Three references.  (1) The group law of oracle.curves: the bases of a case are [b_i] g for integers b_i the case knows (made by
ark355_fixed_base_mul_dev, b_i = 0 giving the point at infinity), so a segment's result is [sum_i k_i b_i mod r] g -- one scalar
multiplication of the oracle, used for every segment of at most 65 scalars.  (2) ark355_msm_dev segment by segment, at every length.
(3) The same batch under MSM_BATCH_SMALL_MAX = 0, which runs no line of the short route.

A design is asserted on integers before the library is called: `digits` below recodes a scalar into the signed window digits of the
handle's plan (read back through ark355_diag_msm_sort) from their definition alone, and the designed scalars are checked with it.

`io` carries the tier's device memory, as in tests/sr1cs_cases.py.  Not reachable at a test's size, and so not covered:
ARK355_ENOMEM and a handle of another device."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import mle_open_cases as mo
import poly_cases as pc
import quotient_cases as qc
import sumcheck_cases as sk
from oracle import curves as OC
from oracle import serialize as Z
from oracle.fields import BLS12_381, BN254
from snark_amd import _binding as B
from snark_amd.poly import Mle

POLICY = "ARK355_MSM_BATCH_SMALL_MAX"
BATCH_MAX = 4096
ORACLE_MAX = 65
# the borders of a lane pair's wave (32 items), of a wave (64), of a workgroup (256) and the 1024 the issue's provisional default named (the shipped default is 512)
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024)
POLICY_VALUES = (-3, 0, 1, 64, 1024, 1 << 14, 10 ** 6)
# The shipped default is 512.  A case that is about the short route sets the policy to its ceiling, so that every segment up to 2^14
# scalars -- the 1023 and 1024 of LENGTHS, the 1024 of PLAN_LENGTHS, 64 x 1024 -- takes it; the default itself is what policy_case
# (-3) and open_case (-1) run under.
SHORT_ALL = 1 << 14
# (bases, MSM_C, TABLE_STRIDE, PACK_ROWS): every value of each knob at least once, both handle sizes, both row formats at a stride
PLANS = ((1024, 4, 1, 0), (1024, 8, 2, 1), (1024, 13, 3, 1), (1024, 17, 2, 0), (4096, 13, 1, 0), (4096, 17, 3, 1))
PLAN_LENGTHS = (5, 64, 1024)

unraw, mont, expect_refusal = pc.unraw, qc.mont, pc.expect_refusal


# ---- integers ----------------------------------------------------------------------------------------------------------------------
def digits(r, k, c, windows, negate_high):
    """(flip, [d_0 .. d_{windows-1}]): k' = sum_w d_w 2^(c w) with -2^(c-1) < d_w <= 2^(c-1), k' = r - k (flip) for k above (r - 1) / 2
    under negate_high and k otherwise"""
    flip = bool(negate_high) and k > (r - 1) // 2
    rest, out, B = (r - k if flip else k), [], 1 << (c - 1)
    for _ in range(windows):
        d = rest & ((1 << c) - 1)
        if d > B:
            d -= 1 << c
        out.append(d)
        rest = (rest - d) >> c
    assert rest == 0, "the plan's windows do not hold the scalar"
    assert sum(d << (c * w) for w, d in enumerate(out)) == (r - k if flip else k)
    return flip, out


def designed_scalars(r, c, windows, negate_high):
    """name -> scalar, each checked against `digits`"""
    B, top = 1 << (c - 1), ((r - 1) // 2 if negate_high else r - 1)
    full = max(w for w in range(1, windows + 1) if sum(B << (c * i) for i in range(w)) <= top)
    all_b = sum(B << (c * i) for i in range(full))
    chain = max(w for w in range(1, windows) if 1 + sum(B << (c * i) for i in range(w)) <= top)
    all_b1 = 1 + sum(B << (c * i) for i in range(chain))
    out = {"0": 0, "1": 1, "r-1": r - 1, "(r-1)/2": (r - 1) // 2, "(r+1)/2": (r + 1) // 2, "all B": all_b, "all B+1": all_b1}
    for w in (1, 2, windows - 1):
        out["2^%d-1" % (c * w)] = (1 << (c * w)) - 1
        out["2^%d" % (c * w)] = 1 << (c * w)
    assert digits(r, all_b, c, windows, negate_high) == (False, [B] * full + [0] * (windows - full))
    # B + 1 in every window once the carry has arrived: each becomes -(B - 1) and carries on, the last carry is a digit 1
    assert digits(r, all_b1, c, windows, negate_high) == (False, [-(B - 1)] * chain + [1] + [0] * (windows - chain - 1))
    assert digits(r, (r + 1) // 2, c, windows, negate_high)[0] == bool(negate_high)
    assert digits(r, (r - 1) // 2, c, windows, negate_high)[0] is False
    assert digits(r, (1 << c) - 1, c, windows, negate_high)[1][:2] == [-1, 1]
    return out


# ---- bases -------------------------------------------------------------------------------------------------------------------------
class Side:
    """one curve and group: the oracle's group, the library's bytes"""

    def __init__(self, lib, ctx, C, io, group):
        self.lib, self.ctx, self.C, self.io, self.group = lib, ctx, C, io, group
        self.G = OC.g1(C) if group == 1 else OC.g2(C)
        self.gen = C.g1_gen if group == 1 else C.g2_gen
        self.enc = Z.g1_raw if group == 1 else Z.g2_raw
        self.size = lib.sizes(C.curve_id)["g1" if group == 1 else "g2"]
        self.inf = bytes(self.size)
        self.handles = []

    def point_of(self, scalar):
        s = scalar % self.C.r
        return self.enc(self.C, self.G.mul(self.gen, s) if s else None)

    def points(self, mults):
        """[b] g for every b of mults, by the library's fixed-base multiplication; b = 0 is the point at infinity"""
        d_b, keep = self.io.to_dev(unraw(m % self.C.r for m in mults))
        out = self.lib.fixed_base_mul_dev(self.ctx, self.C.curve_id, self.group, self.enc(self.C, self.gen), d_b, len(mults), False, self.size)
        for i in (0, len(mults) - 1):
            assert out[i * self.size:(i + 1) * self.size] == self.point_of(mults[i]), "the bases themselves"
        return out

    def load(self, points, n):
        h = self.lib.bases_load(self.ctx, self.C.curve_id, self.group, points[:n * self.size], n)
        self.handles.append(h)
        return h

    def plan(self, h, n):
        """the plan an MSM of n scalars over handle h runs under"""
        return self.lib.diag_msm_sort(self.ctx, self.C.curve_id, bytes(32 * n), n, 0, bases=h, arrays=False)

    def free(self):
        for h in self.handles:
            self.lib.dll.ark355_bases_free(h)
        self.handles = []


class Batch:
    """segments (handle, multipliers of its bases, scalars) and the three references"""

    def __init__(self, side, use_mont):
        self.side, self.use_mont, self.segs, self.keep = side, use_mont, [], []

    def add(self, h, mults, scalars):
        C = self.side.C
        d = None
        if scalars:
            d, k = self.side.io.to_dev((mont(C, scalars) if self.use_mont else unraw(scalars)) + mo.A5)
            self.keep.append((k, len(scalars)))
        self.segs.append((h, mults, list(scalars), d))

    def run(self):
        s = self.side
        out = s.lib.msm_batch_dev(s.ctx, [g[0] for g in self.segs], [g[3] for g in self.segs], [len(g[2]) for g in self.segs],
                                  self.use_mont, s.size)
        return [out[i * s.size:(i + 1) * s.size] for i in range(len(self.segs))]

    def check(self, tag, policy=None, got=None):
        """the batch against the oracle (short segments), against ark355_msm_dev (every segment) and -- with `policy` -- run with
        the short route open to every segment up to 2^14 scalars and compared with itself with the route switched off; without
        `policy` the batch runs under whatever the context holds.  Returns the points"""
        s = self.side
        if policy is not None:
            policy.setenv(POLICY, SHORT_ALL)
            assert s.lib.ctx_get_policy(s.ctx, "MSM_BATCH_SMALL_MAX") == SHORT_ALL
        got = got or self.run()
        for i, (h, mults, scalars, d) in enumerate(self.segs):
            where = (tag, "segment %d of %d scalars" % (i, len(scalars)))
            if len(scalars) <= ORACLE_MAX:
                assert got[i] == s.point_of(sum(k * b for k, b in zip(scalars, mults))), (where, "against the oracle")
            ref = s.lib.msm_dev(s.ctx, h, d, len(scalars), self.use_mont, s.size) if scalars else s.lib.msm_dev(s.ctx, h, 0, 0, 0, s.size)
            assert got[i] == ref, (where, "against ark355_msm_dev")
        if policy is not None:
            policy.setenv(POLICY, 0)
            off = self.run()
            policy.setenv(POLICY, -1)
            assert off == got, (tag, "against MSM_BATCH_SMALL_MAX = 0", [i for i in range(len(got)) if off[i] != got[i]])
        for k, n in self.keep:
            assert s.io.read(k, 32 * n + 32)[32 * n:] == mo.A5, (tag, "the scalars were written")
        return got


def random_mults(C, rnd, n, holes=True):
    """random multipliers; every 11th base is the point at infinity"""
    return [0 if holes and i % 11 == 5 else rnd.randrange(1, C.r) for i in range(n)]


# ---- 1: lengths, designed scalars --------------------------------------------------------------------------------------------------
def lengths_case(lib, ctx, C, io, policy, group, use_mont):
    """every length of LENGTHS in ONE batch over a handle of 1024 bases with points at infinity mixed in; the designed scalars lead
    every segment that holds them; then count 1 at a lane-pair border"""
    rnd = random.Random("msm-batch/lengths/%d/%d" % (group, C.curve_id))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        mults = random_mults(C, rnd, 1024)
        h = s.load(s.points(mults), 1024)
        plan = s.plan(h, 1024)
        # the planner's own choice for 1024 bases: 8 bits over 255-bit scalars, 5 over 254-bit ones (51 windows)
        assert (plan["c"], plan["wstride"], plan["negate_high"], plan["row_stride"]) == (8 if C is BLS12_381 else 5, 1, 0, 1024), plan
        design = list(designed_scalars(p, plan["c"], plan["windows"], plan["negate_high"]).values())
        b = Batch(s, use_mont)
        for n in LENGTHS:
            scalars = (design + [rnd.randrange(p) for _ in range(n)])[:n] if n >= 31 else [(p - 1, (p - 1) // 2, (p + 1) // 2)[i] for i in range(n)]
            b.add(h, mults, scalars)
        got = b.check((C.name, group, "lengths"), policy)
        assert got[0] == s.inf
        one = Batch(s, use_mont)
        one.add(h, mults, b.segs[5][2])
        assert one.check((C.name, group, "count 1")) == [got[5]]
    finally:
        s.free()


# ---- 2: the opening's shape, a repeated handle ---------------------------------------------------------------------------------------
def opening_shape_case(lib, ctx, C, io, policy, group, top=10):
    """2^top, .., 2, 1 scalars against handles of exactly as many bases: on BLS12-381 two window sizes in one call"""
    rnd = random.Random("msm-batch/opening/%d/%d" % (group, C.curve_id))
    s = Side(lib, ctx, C, io, group)
    try:
        mults = random_mults(C, rnd, 1 << top)
        pts = s.points(mults)
        b = Batch(s, 1)
        cs = set()
        for j in range(top, -1, -1):
            h = s.load(pts, 1 << j)
            cs.add(s.plan(h, 1 << j)["c"])
            b.add(h, mults, [rnd.randrange(C.r) for _ in range(1 << j)])
        assert top < 10 or cs == ({4, 8} if C is BLS12_381 else {5}), cs      # BN254's planner picks 5 bits at every one of these sizes
        b.check((C.name, group, "the opening's shape"), policy)
    finally:
        s.free()


def repeated_handle_case(lib, ctx, C, io, policy, group, count=64, n=16):
    """one handle `count` times; an all-zero segment and a cancelling one between neighbours that are not"""
    rnd = random.Random("msm-batch/repeat/%d/%d" % (group, C.curve_id))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        mults = random_mults(C, rnd, 64, holes=False)
        mults[1] = p - mults[0]                                 # base 1 = -base 0
        h = s.load(s.points(mults), 64)
        b = Batch(s, 0)
        for i in range(count):
            scalars = [rnd.randrange(p) for _ in range(n)]
            if i == 7:
                scalars = [0] * n
            if i == 9:
                scalars = [scalars[0], scalars[0]] + [0] * (n - 2)
            b.add(h, mults, scalars)
        assert sum(k * m for k, m in zip(b.segs[9][2], mults)) % p == 0
        got = b.check((C.name, group, "one handle %d times" % count), policy)
        assert got[7] == s.inf and got[9] == s.inf and s.inf not in (got[6], got[8], got[10])
    finally:
        s.free()


# ---- 3: designed bases -------------------------------------------------------------------------------------------------------------
def designed_bases_case(lib, ctx, C, io, policy, group):
    """all bases equal with all scalars equal: every chain step and every butterfly step is a doubling; P, -P alternating: every
    pair cancels and the sums pass through infinity; the same with infinity mixed in"""
    rnd = random.Random("msm-batch/bases/%d/%d" % (group, C.curve_id))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        m, k = rnd.randrange(1, p), rnd.randrange(1, p)
        equal = [m] * 257
        alt = [(m, p - m)[i & 1] for i in range(256)]
        holes = [0 if i % 3 == 2 else (m, p - m)[(i // 3) & 1] for i in range(255)]
        assert sum(alt) % p == 0 and sum(holes[:252]) % p == 0
        h_eq, h_alt, h_holes = s.load(s.points(equal), 257), s.load(s.points(alt), 256), s.load(s.points(holes), 255)
        b = Batch(s, 1)
        for n in (2, 33, 64, 65, 257):
            b.add(h_eq, equal, [k] * n)
        for n in (2, 64, 256):
            b.add(h_alt, alt, [k] * n)
        b.add(h_alt, alt, [k] * 33)                              # one base left over
        b.add(h_holes, holes, [k] * 252)
        b.add(h_holes, holes, [k] * 64)                          # 21 triples (m, m, 0) / (-m, -m, 0), then one -m
        b.add(h_alt, alt, [rnd.randrange(p) for _ in range(64)])
        got = b.check((C.name, group, "designed bases"), policy)
        assert got[0] == s.point_of(2 * k * m) and got[4] == s.point_of(257 * k * m)
        assert got[5:8] == [s.inf] * 3 and got[8] == s.point_of(k * m) and got[9] == s.inf
        assert got[10] == s.point_of(k * m) and got[11] != s.inf
    finally:
        s.free()


# ---- 4: plans ------------------------------------------------------------------------------------------------------------------------
def plan_case(lib, ctx, C, io, policy, group, nb, c, stride, pack, lengths=PLAN_LENGTHS):
    """a handle of nb bases loaded under MSM_C, TABLE_STRIDE and PACK_ROWS; 5, 64 and 1024 scalars in one batch, with the scalars
    designed for THIS plan's windows in each"""
    rnd = random.Random("msm-batch/plan/%d/%d/%d/%d/%d/%d" % (group, C.curve_id, nb, c, stride, pack))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        mults = random_mults(C, rnd, nb)
        pts = s.points(mults)
        for name, v in (("MSM_C", c), ("TABLE_STRIDE", stride), ("PACK_ROWS", pack)):
            policy.setenv("ARK355_" + name, v)
        h = s.load(pts, nb)
        policy.restore()
        policy.saved = []
        windows = -(-(C.r.bit_length() + 1) // c)
        negate = C is BLS12_381 and c == 17
        if negate:
            windows -= 1
        for n in lengths:
            plan = s.plan(h, n)
            assert (plan["c"], plan["windows"], plan["wstride"], plan["negate_high"], plan["row_stride"]) == \
                (c, windows, min(stride, windows), int(negate), nb), (plan, "not the plan the case was designed for")
        design = designed_scalars(p, c, windows, negate)
        b = Batch(s, 1)
        b.add(h, mults, [design["r-1"], design["(r+1)/2"], design["all B"], design["all B+1"], rnd.randrange(p)])
        for n in lengths[1:]:
            b.add(h, mults, (list(design.values()) + [rnd.randrange(p) for _ in range(n)])[:n])
        b.check((C.name, group, "plan", nb, c, stride, pack), policy)
    finally:
        s.free()


# ---- 5: the policy -------------------------------------------------------------------------------------------------------------------
def policy_case(lib, ctx, C, io, policy, group=1, lengths=(0, 1, 31, 64, 65)):
    """no value changes a byte; at 64 the batch mixes both routes"""
    rnd = random.Random("msm-batch/policy/%d/%d" % (group, C.curve_id))
    s = Side(lib, ctx, C, io, group)
    try:
        assert lib.ctx_get_policy(ctx, "MSM_BATCH_SMALL_MAX") < 0, "the context does not start at the default"
        mults = random_mults(C, rnd, 65)
        h = s.load(s.points(mults), 65)
        b = Batch(s, 0)
        for n in lengths:
            b.add(h, mults, [rnd.randrange(C.r) for _ in range(n)])
        want = b.check((C.name, group, "policy"), policy)
        assert lib.ctx_get_policy(ctx, "MSM_BATCH_SMALL_MAX") == -1
        assert any(1 <= n <= 64 for n in lengths) and any(n > 64 for n in lengths)
        for value in POLICY_VALUES:
            policy.setenv(POLICY, value)
            assert lib.ctx_get_policy(ctx, "MSM_BATCH_SMALL_MAX") == value
            assert b.run() == want, (C.name, "MSM_BATCH_SMALL_MAX = %d changed the bytes" % value)
        policy.setenv(POLICY, -1)
    finally:
        s.free()


# ---- 6: the opening and the commitments ----------------------------------------------------------------------------------------------
def open_case(lib, ctx, C, io, policy, group, v):
    """ark355_mle_open_dev: the same bytes with the short route off and at the default, and the oracle's proof (mle_open_cases)"""
    rnd = random.Random("msm-batch/open/%d/%d/%d" % (group, v, C.curve_id))
    p = C.r
    key = mo.Key(lib, ctx, C, io, group, [rnd.randrange(1, p) for _ in range(v)])
    try:
        f, point = [rnd.randrange(p) for _ in range(1 << v)], [rnd.randrange(p) for _ in range(v)]
        d_f, k0 = io.to_dev(mont(C, f))
        runs = {}
        for value in (0, -1, 3):
            policy.setenv(POLICY, value)
            runs[value] = key.mle.open_dev(key.levels, d_f, v, point, group)
        policy.setenv(POLICY, -1)
        assert runs[0] == runs[-1] == runs[3], (C.name, group, v, "the opening depends on MSM_BATCH_SMALL_MAX")
        scalars, y = mo.open_scalars(p, f, point, key.t)
        assert runs[-1] == (b"".join(key.point_of(x) for x in scalars), mont(C, [y])), (C.name, group, v, "against the oracle")
    finally:
        key.free()


def commit_case(lib, ctx, C, io, group, v=5, count=3):
    """Mle.commit_dev: `count` resident tables, one key, against ark355_msm_dev table by table and the oracle"""
    rnd = random.Random("msm-batch/commit/%d/%d" % (group, C.curve_id))
    p, N = C.r, 1 << v
    key = mo.Key(lib, ctx, C, io, group, [rnd.randrange(1, p) for _ in range(v)])
    try:
        f = [rnd.randrange(p) for _ in range(count * N)]
        f[N:2 * N] = [0] * N
        d_f, k0 = io.to_dev(mont(C, f))
        got = key.mle.commit_dev(key.commit, d_f, v, count, group)
        want = b"".join(lib.msm_dev(ctx, key.commit, d_f + 32 * N * k, N, 1, key.size) for k in range(count))
        assert got == want
        assert got == b"".join(key.point_of(sk.eval_def(p, f[k * N:(k + 1) * N], key.t)) for k in range(count))
        assert got[key.size:2 * key.size] == bytes(key.size)
    finally:
        key.free()


# ---- 7: robustness -------------------------------------------------------------------------------------------------------------------
def small_batch(s, rnd, h, mults, lengths, use_mont=0):
    b = Batch(s, use_mont)
    for n in lengths:
        b.add(h, mults, [rnd.randrange(s.C.r) for _ in range(n)])
    return b


def dirty_sequence(lib, ctx, C, io):
    """in a fresh context: a large batch, a small one on another group, a refusal, the large one again: every step against the
    references, the last against the first"""
    rnd = random.Random("msm-batch/dirty/%d" % C.curve_id)
    s1, s2 = Side(lib, ctx, C, io, 1), Side(lib, ctx, C, io, 2)
    try:
        m1, m2 = random_mults(C, rnd, 300), random_mults(C, rnd, 40)
        h1, h2 = s1.load(s1.points(m1), 300), s2.load(s2.points(m2), 40)
        big = small_batch(s1, rnd, h1, m1, (300, 64, 1, 257), 1)
        first = big.check((C.name, "large batch"))
        small_batch(s2, rnd, h2, m2, (3, 0, 40)).check((C.name, "small batch on G2"))
        small_batch(s1, rnd, h1, m1, (2,)).check((C.name, "one segment of two"))
        expect_refusal(lib, ctx, lambda: lib.msm_batch_dev(ctx, [h1, h2], [big.segs[0][3]] * 2, [1, 1], 0, s1.size), needle="segment 1")
        assert big.check((C.name, "large batch again")) == first
    finally:
        s1.free()
        s2.free()


def interleaved_case(lib, ctx, C, io):
    """ark355_msm_dev, ark355_mle_quotients_fr_dev and an opening between two batches: unchanged bytes"""
    rnd = random.Random("msm-batch/interleaved/%d" % C.curve_id)
    p = C.r
    s = Side(lib, ctx, C, io, 1)
    key = mo.Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(4)])
    try:
        mults = random_mults(C, rnd, 100)
        h = s.load(s.points(mults), 100)
        b = small_batch(s, rnd, h, mults, (100, 5, 33))
        first = b.check((C.name, "first batch"))
        other = [rnd.randrange(p) for _ in range(64)]
        d_o, k = io.to_dev(unraw(other))
        assert lib.msm_dev(ctx, h, d_o, 64, 0, s.size) == s.point_of(sum(a * m for a, m in zip(other, mults)))
        want, vals = mo.layout_ref(p, [other[:16], other[16:32]], [3, 5, 7, 11])
        assert mo.dev_quot(lib, ctx, C, io, unraw(other[:32]), 4, 2, [3, 5, 7, 11]) == (unraw(want), unraw(vals))
        mo.check_open(key, io, other[:16], [rnd.randrange(p) for _ in range(4)], (C.name, "an opening between two batches"))
        assert b.run() == first, (C.name, "other entries between two batches changed the bytes")
    finally:
        key.free()
        s.free()


def refusals_case(lib, ctx, C, io):
    """every refusal a test's size reaches, by code and with a message that names the segment, each followed by a good call"""
    rnd = random.Random("msm-batch/refusals/%d" % C.curve_id)
    d, vp = lib.dll, ctypes.c_void_p
    O = BN254 if C is BLS12_381 else BLS12_381
    s, s2, alien = Side(lib, ctx, C, io, 1), Side(lib, ctx, C, io, 2), Side(lib, ctx, O, io, 1)
    try:
        mults = random_mults(C, rnd, 8)
        h = s.load(s.points(mults), 8)
        h2 = s2.load(s2.points(mults), 8)
        ha = alien.load(alien.points(mults), 8)
        good_batch = small_batch(s, rnd, h, mults, (8, 3, 0))
        want = good_batch.check((C.name, "before the refusals"))
        d_s = good_batch.segs[0][3]
        out = np.zeros(4 * s2.size, dtype=np.uint8)
        ptr = out.ctypes.data_as(vp)
        arr = lambda xs: (vp * len(xs))(*xs)                                     # noqa: E731
        u64 = lambda xs: (ctypes.c_uint64 * len(xs))(*xs)                        # noqa: E731
        fn = d.ark355_msm_batch_dev

        def refused(rc, needle=None, message=True):
            assert rc == B.EINVAL, rc
            if message:
                msg = d.ark355_last_error(ctx).decode()
                assert msg and (needle is None or needle in msg), msg
            assert good_batch.run() == want, "the context after a refusal"

        H, P, N = arr([h, h, h]), arr([d_s, d_s, d_s]), u64([8, 3, 1])
        refused(fn(None, H, P, N, 3, 0, ptr), message=False)
        refused(fn(ctx, None, P, N, 3, 0, ptr), "NULL")
        refused(fn(ctx, H, None, N, 3, 0, ptr), "NULL")
        refused(fn(ctx, H, P, None, 3, 0, ptr), "NULL")
        refused(fn(ctx, H, P, N, 3, 0, None), "NULL")
        refused(fn(ctx, H, P, N, BATCH_MAX + 1, 0, ptr), "ARK355_MSM_BATCH_MAX")
        refused(fn(ctx, arr([h, None, h]), P, u64([8, 0, 1]), 3, 0, ptr), "segment 1: the handle is NULL")
        refused(fn(ctx, arr([h, h, ha]), P, N, 3, 0, ptr), "segment 2: the handle belongs to another curve")
        refused(fn(ctx, arr([h, h2, h]), P, N, 3, 0, ptr), "segment 1: the handle is of another group")
        refused(fn(ctx, H, P, u64([8, 9, 1]), 3, 0, ptr), "segment 1: 9 scalars, more than the handle's 8 bases")
        refused(fn(ctx, H, arr([d_s, d_s, None]), N, 3, 0, ptr), "segment 2: d_scalars is NULL")
        assert not out.any(), "a refused batch wrote"
        assert fn(ctx, None, None, None, 0, 0, None) == B.OK                       # count = 0: nothing to do
        own = arr([good_batch.segs[0][3], good_batch.segs[1][3], None])
        assert fn(ctx, H, own, u64([8, 3, 0]), 3, 0, ptr) == B.OK                # an empty segment reads no scalars
        assert out.tobytes()[:3 * s.size] == b"".join(want) and not out[3 * s.size:].any()
    finally:
        s.free()
        s2.free()
        alien.free()


# ---- [GPU only] ----------------------------------------------------------------------------------------------------------------------
def many_segments_case(lib, ctx, C, io, policy, group, count, n, nb=None):
    """`count` segments of n scalars over one handle, against the same batch with the short route off (ark355_msm_dev's pipeline
    segment by segment) and the oracle on four segments"""
    rnd = random.Random("msm-batch/many/%d/%d/%d/%d" % (group, C.curve_id, count, n))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        nb = nb or n
        mults = random_mults(C, rnd, nb)
        h = s.load(s.points(mults), nb)
        rows = np.random.default_rng(count + n + C.curve_id).integers(0, 256, size=(count * n, 32), dtype=np.uint8)
        rows[:, 31] &= (1 << ((p >> 248).bit_length() - 1)) - 1            # below r
        d_s, keep = io.to_dev(rows.tobytes())
        args = ([h] * count, [d_s + 32 * n * i for i in range(count)], [n] * count, 0, s.size)
        policy.setenv(POLICY, SHORT_ALL)
        got = lib.msm_batch_dev(ctx, *args)
        policy.setenv(POLICY, 0)
        off = lib.msm_batch_dev(ctx, *args)
        policy.setenv(POLICY, -1)
        assert got == off, (C.name, group, count, n, [i for i in range(count) if got[i * s.size:(i + 1) * s.size] != off[i * s.size:(i + 1) * s.size]][:8])
        for i in (0, 1, count // 2, count - 1):
            ks = [int.from_bytes(rows[i * n + j].tobytes(), "little") for j in range(n)]
            assert got[i * s.size:(i + 1) * s.size] == s.point_of(sum(k * b for k, b in zip(ks, mults))), (C.name, group, "segment %d against the oracle" % i)
    finally:
        s.free()


def long_between_short_case(lib, ctx, C, io, policy, group, long_n=1 << 15):
    """one segment of 2^15 scalars -- beyond every value of the policy -- between short ones"""
    rnd = random.Random("msm-batch/long/%d/%d" % (group, C.curve_id))
    p = C.r
    s = Side(lib, ctx, C, io, group)
    try:
        mults = random_mults(C, rnd, long_n)
        h = s.load(s.points(mults), long_n)
        b = Batch(s, 1)
        for n in (33, long_n, 1, 1024, 0, 64):
            b.add(h, mults, [rnd.randrange(p) for _ in range(n)])
        got = b.check((C.name, group, "a long segment between short ones"), policy)
        assert got[1] == s.point_of(sum(k * m for k, m in zip(b.segs[1][2], mults)))
    finally:
        s.free()
