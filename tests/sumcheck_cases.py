"""Cases of the multilinear primitives and of the sum-check of a predicate, shared by the CPU-emulator tier and the GPU tier
(tests/test_emul_sumcheck.py, tests/test_gpu_sumcheck.py): ark355_mle_eq_fr, ark355_mle_fix_fr, ark355_mle_eval_fr, their `_dev`
variants, ark355_gr1cs_sumcheck_begin_dev, ark355_sumcheck_round / _finish / _info / _free (include/ark355.h "Multilinear
extensions" and "Sum-check of a GR1CS predicate").  Every comparison is byte for byte or an exact identity of integers.

The reference is plain big-integer code holding the header's definitions written as sums over the hypercube (eq_ref, eval_def,
round_ref), the folding rule (fold_ref), and a verifier (verify) that interpolates g_j at r_j from its D + 1 values over 0 .. D,
checks g_1(0) + g_1(1) = S, the chain g_{j+1}(0) + g_{j+1}(1) = g_j(r_j) and the last identity against the finals.

Fixing a variable is linear in the table, so fix / eval are compared on the raw Montgomery images (v R mod r) with the canonical
point, as tests/evals_cases.py does; eq and the rounds are not linear and are compared through real conversions.

The `_dev` variants always write into buffers pre-filled with 0xA5 that are one element longer than needed, and the extra element
is checked after every call.  `io` carries the tier's device memory, as in tests/sr1cs_cases.py.  Not reachable at a test's size,
and so not covered: ARK355_ENOMEM, and the refusal of a handle of another device (one device per tier)."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import evals_cases as ec
import gr1cs_cases as gc
import poly_cases as pc
import quotient_cases as qc
from helpers import z_bytes
from snark_amd import _binding as B
from snark_amd.poly import Sumcheck

POLICY = "ARK355_SUMCHECK_LANE_PAIRS"
P_DEFAULT = 1                               # SUMCHECK_LANE_PAIRS's default (snark_amd/csrc/sumcheck_impl.cuh): one element a lane
P_OTHER = 4                                 # the other side of the byte comparison at 2^20 entries
MAX_COUNT = 1024                            # ARK355_POLY_MAX_COUNT
MAX_POINTS = 32                             # ARK355_SUMCHECK_MAX_POINTS
A5 = b"\xA5" * 32
# Primitives.  fix: a lane owns P outputs of a halving (the first has 2^(v-1)), a wave 64 P, a workgroup 256 P.  P = 1, the default:
# one wave and two at 64 / 128 outputs (v = 7, 8), one workgroup and two at 256 / 512 (v = 9, 10).  eq: a lane owns 8 outputs (v = 3,
# 4), a wave 512 (v = 9, 10), a workgroup 2048 (v = 11, 12).  P = 2: a lane border at 2 / 4 outputs (v = 2, 3), a wave border at 128 /
# 256 (v = 8, 9), a workgroup border at 512 / 1024 (v = 10, 11).  The later halvings of every call cross the smaller borders on the
# way down.
MLE_SHAPES_DEFAULT = (0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13)
MLE_SHAPES_P2 = (2, 3, 8, 9, 10, 11)
# Rounds.  The round kernel's workgroup owns lanes x P output pairs; for the R1CS shape (10 slots with a weight, 9 without) lanes =
# 128: round 1 of v has 2^(v-1) pairs.  P = 1, the default: one wave and two at 64 / 128 pairs (v = 7, 8), one workgroup and two at
# 128 / 256 pairs (v = 8, 9).  P = 2: a lane border at 2 / 4 pairs (v = 2, 3), a wave of 128 pairs (v = 8, 9), a workgroup of 256 (v =
# 9, 10).  P = 3: a workgroup of 384 pairs, v = 9 / 10.  The later rounds of every run cross the smaller borders on the way down.
ROUND_SHAPES_DEFAULT = (0, 1, 2, 3, 4, 7, 8, 9, 10)
ROUND_SHAPES_P2 = (2, 3, 8, 9, 10)
ROUND_SHAPES_P3 = (9, 10)

xb = pc.xb
raw = pc.raw
unraw = pc.unraw
expect_refusal = pc.expect_refusal
mont = qc.mont
fr_list = qc.fr_list


def point_bytes(point):
    return b"".join(xb(x) for x in point)


# ---- the reference: plain integers -----------------------------------------------------------------------------------------------
def eq_ref(p, point):
    """out[i] = prod_j (b_j x_j + (1 - b_j)(1 - x_j)), i = sum_j b_j 2^j: variable j is index bit j"""
    out = [1]
    for x in point:
        out = [o * (1 - x) % p for o in out] + [o * x % p for o in out]
    return out


def fold_ref(p, f, r):
    return [(f[2 * i] + r * (f[2 * i + 1] - f[2 * i])) % p for i in range(len(f) // 2)]


def fix_ref(p, f, point):
    for r in point:
        f = fold_ref(p, f, r)
    return f


def eval_def(p, f, point):
    """the extension by its definition: a sum over the hypercube"""
    return sum(fi * ei for fi, ei in zip(f, eq_ref(p, point))) % p


def claim_ref(p, terms, T, W):
    """S = sum_i W[i] P(T_0[i], .., T_{t-1}[i])"""
    return sum((W[i] if W else 1) * gc.residual(p, terms, [t[i] for t in T]) for i in range(len(T[0]))) % p


def round_ref(p, terms, T, W, D):
    """g[X] = sum_i Wx P(A_0, .., A_{t-1}) over the pairs (2i, 2i+1) of the state, X = 0 .. D"""
    g = []
    for X in range(D + 1):
        acc = 0
        for i in range(len(T[0]) // 2):
            vals = [(t[2 * i] + X * (t[2 * i + 1] - t[2 * i])) % p for t in T]
            wx = (W[2 * i] + X * (W[2 * i + 1] - W[2 * i])) % p if W else 1
            acc += wx * gc.residual(p, terms, vals)
        g.append(acc % p)
    return g


def prover_ref(p, terms, T, W, D, challenges):
    """(messages, finals) of the whole run: the state is folded by fold_ref between two rounds"""
    msgs = []
    for j in range(len(challenges)):
        if j:
            T, W = [fold_ref(p, t, challenges[j - 1]) for t in T], (fold_ref(p, W, challenges[j - 1]) if W else None)
        msgs.append(round_ref(p, terms, T, W, D))
    if challenges:
        T, W = [fold_ref(p, t, challenges[-1]) for t in T], (fold_ref(p, W, challenges[-1]) if W else None)
    return msgs, [t[0] for t in T] + [W[0] if W else 1]


def interpolate_at(p, g, r):
    """the polynomial of degree <= D through (X, g[X]), X = 0 .. D, at r"""
    D = len(g) - 1
    acc = 0
    for X in range(D + 1):
        num, den = 1, 1
        for Y in range(D + 1):
            if Y != X:
                num = num * (r - Y) % p
                den = den * (X - Y) % p
        acc += g[X] * num * pow(den, -1, p)
    return acc % p


def verify(p, terms, S, msgs, challenges, finals, tag):
    """the verifier of IPForMLSumcheck: S is the claim, or None when nobody summed the hypercube"""
    expected = S
    for j, (g, r) in enumerate(zip(msgs, challenges)):
        if expected is not None:                               # a message of one point (D = 0) is a constant: g(1) = g(0)
            assert (g[0] + interpolate_at(p, g, 1)) % p == expected, (tag, "g_%d(0) + g_%d(1) is not the running claim" % (j + 1, j + 1))
        expected = interpolate_at(p, g, r)
    want = finals[-1] * gc.residual(p, terms, finals[:-1]) % p
    if expected is not None:
        assert want == expected, (tag, "the last identity g_v(r_v) = W P(T_0, ..) fails")


# ---- primitives ------------------------------------------------------------------------------------------------------------------
def dev_eq(lib, ctx, C, io, point):
    N = 1 << len(point)
    d_o, k = io.alloc((N + 1) * 32)
    lib.mle_eq_fr_dev(ctx, C.curve_id, len(point), point_bytes(point), d_o)
    got = io.read(k, (N + 1) * 32)
    assert got[N * 32:] == A5, "eq wrote behind its output"
    return got[:N * 32]


def dev_fix(lib, ctx, C, io, fb, v, count, point, eval_entry=False):
    k = len(point)
    size = (count << (v - k)) * 32
    d_f, k0 = io.to_dev(fb + A5)
    d_o, k1 = io.alloc(size + 32)
    if eval_entry:
        lib.mle_eval_fr_dev(ctx, C.curve_id, d_f, v, count, point_bytes(point), d_o)
    else:
        lib.mle_fix_fr_dev(ctx, C.curve_id, d_f, v, count, point_bytes(point), k, d_o)
    got = io.read(k1, size + 32)
    assert got[size:] == A5, "fix / eval wrote behind its output"
    assert io.read(k0, len(fb) + 32) == fb + A5, "fix / eval changed its input"
    return got[:size]


def mle_points(C, rnd, v):
    p = C.r
    return {"random": [rnd.randrange(p) for _ in range(v)], "zeros": [0] * v, "ones": [1] * v, "r-1": [p - 1] * v,
            "boolean": [rnd.randrange(2) for _ in range(v)], "mixed": [(0, 1, p - 1, rnd.randrange(p))[j % 4] for j in range(v)]}


def primitives_case(lib, ctx, C, io, policy, P, v, counts=(1, 3)):
    """eq, fix for every k and eval against the definitions, host and `_dev` forms, at P outputs a lane"""
    p = C.r
    policy.setenv(POLICY, P)
    rnd = random.Random("mle/%d/%d/%d" % (v, P, C.curve_id))
    N = 1 << v
    pts = mle_points(C, rnd, v)
    names = list(pts) if v <= 9 else ["random", "boolean"]      # above one wave of eq: borders depend on the index, not on the point
    for name in names:
        point = pts[name]
        tag = (C.name, v, P, name)
        want_eq = eq_ref(p, point)
        eqb = dev_eq(lib, ctx, C, io, point)
        assert eqb == mont(C, want_eq), (tag, "eq", qc.first_difference(eqb, mont(C, want_eq)))
        assert lib.mle_eq_fr(ctx, C.curve_id, v, point_bytes(point)) == eqb, (tag, "eq, host form")
        index = None
        if name in ("zeros", "ones", "boolean"):
            index = sum(b << j for j, b in enumerate(point))
            assert want_eq == [int(i == index) for i in range(N)], (tag, "the reference is not an indicator")
        for count in (counts if name in ("random", "boolean") else counts[:1]):
            f = [rnd.randrange(p) for _ in range(count * N)]      # raw images
            fb = unraw(f)
            tables = [f[c * N:(c + 1) * N] for c in range(count)]
            ks = range(v + 1) if (v <= 9 or name == "random") and count == counts[0] else (0, 1, v // 2, v)
            for k in sorted(k for k in set(ks) if k <= v):
                want = unraw(x for t in tables for x in fix_ref(p, t, point[:k]))
                got = dev_fix(lib, ctx, C, io, fb, v, count, point[:k])
                assert got == want, (tag, count, "fix k = %d" % k, qc.first_difference(got, want))
                if k in (0, 1, v):
                    assert lib.mle_fix_fr(ctx, C.curve_id, fb, v, count, point_bytes(point[:k]), k) == want, (tag, "fix, host form", k)
            ev = dev_fix(lib, ctx, C, io, fb, v, count, point, eval_entry=True)
            assert ev == dev_fix(lib, ctx, C, io, fb, v, count, point), (tag, "eval is not fix with k = v")
            assert ev == lib.mle_eval_fr(ctx, C.curve_id, fb, v, count, point_bytes(point)), (tag, "eval, host form")
            assert raw(ev) == [eval_def(p, t, point) for t in tables], (tag, "eval against the sum over the hypercube")
            if index is not None:
                assert raw(ev) == [t[index] for t in tables], (tag, "eval at a Boolean point is not the table's entry")
            # <eq(point), f> = eval(f, point): on the host, with the eq bytes the library returned
            eq_lib = fr_list(C, eqb)
            assert raw(ev) == [sum(a * b for a, b in zip(t, eq_lib)) % p for t in tables], (tag, "<eq, f> != eval")
            if v >= 2:                                           # fix then fix equals one fix
                k1, k2 = 1, v // 2
                mid = dev_fix(lib, ctx, C, io, fb, v, count, point[:k1])
                two = dev_fix(lib, ctx, C, io, mid, v - k1, count, point[k1:k1 + k2])
                assert two == dev_fix(lib, ctx, C, io, fb, v, count, point[:k1 + k2]), (tag, "fix then fix")
    policy.setenv(POLICY, P_DEFAULT)


def lincomb_case(lib, ctx, C, io, v=6):
    """eval is linear in the table: the extension of ark355_poly_lincomb_fr's sum_k c_k f_k at a point is sum_k c_k f~_k(point), on
    real Montgomery values; (<eq(point), f> = eval(f, point) itself is checked on the host in primitives_case)"""
    p = C.r
    rnd = random.Random("mle/lincomb/%d" % C.curve_id)
    N, count = 1 << v, 3
    vals = [rnd.randrange(p) for _ in range(count * N)]
    fb = mont(C, vals)
    scalars = [rnd.randrange(p) for _ in range(count)]
    point = [rnd.randrange(p) for _ in range(v)]
    comb = lib.poly_lincomb_fr(ctx, C.curve_id, fb, N, count, b"".join(xb(s) for s in scalars))
    lhs = fr_list(C, lib.mle_eval_fr(ctx, C.curve_id, comb, v, 1, point_bytes(point)))[0]
    each = fr_list(C, lib.mle_eval_fr(ctx, C.curve_id, fb, v, count, point_bytes(point)))
    assert lhs == sum(s * e for s, e in zip(scalars, each)) % p
    assert each == [eval_def(p, vals[c * N:(c + 1) * N], point) for c in range(count)]


# ---- predicates ------------------------------------------------------------------------------------------------------------------
def predicates(C):
    """name -> (arity, terms): R1CS, SR1CS, the hand-made polynomials of quotient_cases.py (a repeated variable, an exponent 0, a
    constant term, degree 0, 1, 3 and 5, arity 1 and 16) and what they lack: a zero-coefficient term of top degree, and the two
    degrees at which a round takes exactly 32 points, with and without a weight"""
    p = C.r
    s = qc.shapes(C)
    return {
        "r1cs": (3, gc.r1cs_terms(p)), "sr1cs": (2, gc.sr1cs_terms(p)),
        "arity1": s["arity1-N2"][:2], "deg3": s["arity4-deg3-N16"][:2], "deg5": s["deg5-N8"][:2], "deg1": s["deg1-N4"][:2],
        "deg0": s["deg0-N4"][:2], "arity16": s["arity16-deg2-N8"][:2],
        "zero-top": (2, [(0, [(0, 3), (1, 1)]), (3, [(0, 1), (1, 1)]), (p - 2, [(1, 1)]), (11, [])]),
        "deg31": (1, [(1, [(0, 31)]), (p - 5, [(0, 2)])]), "deg30": (2, [(1, [(0, 29), (1, 1)]), (7, [(1, 1)])]),
        "deg32": (1, [(1, [(0, 32)])]), "deg-huge": (1, [(1, [(0, 0xFFFFFFFF), (0, 0xFFFFFFFF)])]),
    }


def load_predicates(lib, ctx, C, names=None):
    """one resident system holding the named predicates (two rows of random matrices each: the sum-check reads only the polynomial)"""
    rnd = random.Random("sumcheck/system/%d" % C.curve_id)
    spec = {}
    for name, (arity, terms) in predicates(C).items():
        if names is None or name in names:
            spec.update(qc.random_spec(C, rnd, name, arity, terms, 2, 9))
    return gc.load(lib, ctx, C, 2, 7, spec)


def degree_of(terms):
    return qc.degree_of(terms)


class Run:
    """one library run over tables of integers: the caller's buffers behind 0xA5, every message and the finals as integers"""

    def __init__(self, lib, ctx, C, io, g, label, T, W, v):
        self.lib, self.ctx, self.C, self.io = lib, ctx, C, io
        self.t, self.v = len(T), v
        self.tb = mont(C, [x for t in T for x in t]) + A5
        self.wb = (mont(C, W) + A5) if W is not None else None
        self.d_t, self.k_t = io.to_dev(self.tb)
        self.d_w, self.k_w = io.to_dev(self.wb) if W is not None else (None, None)
        self.sc = g.sumcheck_dev(label, self.d_t, self.d_w, v)
        self.bytes = []

    def round(self, challenge=None):
        b = self.sc.round(challenge)
        self.bytes.append(b)
        return fr_list(self.C, b)

    def finish(self, challenge=None):
        b = self.sc.finish(challenge)
        self.bytes.append(b)
        return fr_list(self.C, b)

    def untouched(self):
        assert self.io.read(self.k_t, len(self.tb)) == self.tb, "the run wrote the caller's tables"
        if self.wb is not None:
            assert self.io.read(self.k_w, len(self.wb)) == self.wb, "the run wrote the caller's weight"

    def scribble(self):
        """the borrow is over: the caller overwrites its buffers"""
        for keep in (self.k_t, self.k_w):
            if keep is not None:
                (getattr(keep, "fill_", None) or keep.fill)(0x5A)

    def all(self, challenges, scribble_after=2):
        msgs = []
        for j in range(self.v):
            msgs.append(self.round(challenges[j - 1] if j else None))
            if j + 1 == scribble_after:
                self.untouched()
                self.scribble()
        if self.v < scribble_after:
            finals = self.finish(challenges[-1] if self.v else None)
            self.untouched()
            return msgs, finals
        return msgs, self.finish(challenges[-1])

    def close(self):
        self.sc.close()


def random_tables(C, rnd, t, v, weight):
    p, N = C.r, 1 << v
    return [[rnd.randrange(p) for _ in range(N)] for _ in range(t)], ([rnd.randrange(p) for _ in range(N)] if weight else None)


def check_run(lib, ctx, C, io, g, label, terms, T, W, v, rnd, tag, want_S=None):
    """a whole run against prover_ref byte for byte (as integers and as Montgomery bytes), the verifier on the library's messages, info"""
    p = C.r
    D = degree_of(terms) + (1 if W is not None else 0)
    challenges = [rnd.randrange(p) for _ in range(v)]
    run = Run(lib, ctx, C, io, g, label, T, W, v)
    try:
        assert run.sc.info() == (v, len(T), D + 1, 0), (tag, run.sc.info())
        msgs, finals = run.all(challenges)
        assert run.sc.info() == (v, len(T), D + 1, v)
    finally:
        run.close()
    want_msgs, want_finals = prover_ref(p, terms, T, W, D, challenges)
    for j, (got, want) in enumerate(zip(msgs, want_msgs)):
        assert got == want, (tag, "the message of round %d" % (j + 1))
        assert run.bytes[j] == mont(C, want), (tag, "the bytes of round %d" % (j + 1))
    assert len(msgs) == v and finals == want_finals, (tag, "finals")
    assert run.bytes[-1] == mont(C, want_finals)
    S = claim_ref(p, terms, T, W)
    if want_S is not None:
        assert (S == 0) == (want_S == 0), (tag, "the claim", S)
    verify(p, terms, S, msgs, challenges, finals, tag)
    return msgs, finals, challenges


def rounds_case(lib, ctx, C, io, policy, P, name, v, weight):
    arity, terms = predicates(C)[name]
    policy.setenv(POLICY, P)
    rnd = random.Random("sumcheck/%s/%d/%d/%d/%d" % (name, v, P, weight, C.curve_id))
    g = load_predicates(lib, ctx, C, (name,))
    try:
        T, W = random_tables(C, rnd, arity, v, weight)
        check_run(lib, ctx, C, io, g, name, terms, T, W, v, rnd, (C.name, name, v, P, weight))
    finally:
        g.free()
        policy.setenv(POLICY, P_DEFAULT)


# ---- systems: the output of ark355_gr1cs_mat_vec_dev ----------------------------------------------------------------------------------
def system_case(lib, ctx, C, io, name):
    """a satisfying assignment with the weight eq(tau): S = 0 and g_1(0) = g_1(1) = 0 while g_1(2) != 0; one witness changed: S != 0.
    The tables and the weight never leave the device: mat_vec_dev -> mle_eq_fr_dev -> sumcheck -> mle_eval_fr_dev."""
    p = C.r
    ell, w, spec, z, col = qc.satisfied_systems(C)[name]
    rnd = random.Random("sumcheck/system/%s/%d" % (name, C.curve_id))
    g = gc.load(lib, ctx, C, ell, w, spec)
    try:
        label = next(iter(spec))
        arity, terms, mats = spec[label]
        n = len(mats[0])
        v = g.quotient_dims(label)[1]
        N = 1 << v
        tau = [rnd.randrange(p) for _ in range(v)]
        d_w, k_w = io.alloc((N + 1) * 32)
        lib.mle_eq_fr_dev(ctx, C.curve_id, v, point_bytes(tau), d_w)
        W = fr_list(C, io.read(k_w, N * 32))
        assert W == eq_ref(p, tau)
        zbad = list(z)
        zbad[col] = (zbad[col] + 1) % p
        for which, zz in (("satisfied", z), ("broken", zbad)):
            zb = z_bytes(C, zz)
            d_z, k_z = io.to_dev(zb)
            d_t, k_t, N2, vecs = ec.mat_vec_dev(g, io, label, d_z, len(zz), n)
            assert N2 == N
            T = [fr_list(C, b) for b in vecs]
            D = degree_of(terms) + 1
            challenges = [rnd.randrange(p) for _ in range(v)]
            with g.sumcheck_dev(label, d_t, d_w, v) as sc:
                msgs = [fr_list(C, sc.round(challenges[j - 1] if j else None)) for j in range(v)]
                finals = fr_list(C, sc.finish(challenges[-1]))
            want_msgs, want_finals = prover_ref(p, terms, T, W, D, challenges)
            assert msgs == want_msgs and finals == want_finals, (C.name, name, which)
            S = claim_ref(p, terms, T, W)
            verify(p, terms, S, msgs, challenges, finals, (C.name, name, which))
            if which == "satisfied":
                assert S == 0 and msgs[0][0] == 0 and msgs[0][1] == 0 and msgs[0][2] != 0, (C.name, name, msgs[0])
            else:
                assert S != 0 and g.which_is_unsatisfied(zz) is not None
            # cross-entry: the finals are the extensions of the caller's tables at (r_1 .. r_v); the weight's is eq in closed form
            d_e, k_e = io.alloc((arity + 1) * 32)
            lib.mle_eval_fr_dev(ctx, C.curve_id, d_t, v, arity, point_bytes(challenges), d_e)
            got = io.read(k_e, (arity + 1) * 32)
            assert got[arity * 32:] == A5 and fr_list(C, got[:arity * 32]) == finals[:-1]
            closed = 1
            for tj, rj in zip(tau, challenges):
                closed = closed * (tj * rj + (1 - tj) * (1 - rj)) % p
            assert finals[-1] == closed, (C.name, name, "the weight's final is not eq(tau, r)")
    finally:
        g.free()


def restart_case(lib, ctx, C, io, name="r1cs", v=6, weight=True):
    """after j rounds, folding the caller's tables with ark355_mle_fix_fr_dev (k = j) and beginning on the result gives a first message
    byte-identical to round j + 1 of the original run: j = 1, 2, v - 1"""
    p = C.r
    arity, terms = predicates(C)[name]
    rnd = random.Random("sumcheck/restart/%s/%d/%d" % (name, v, C.curve_id))
    g = load_predicates(lib, ctx, C, (name,))
    try:
        T, W = random_tables(C, rnd, arity, v, weight)
        challenges = [rnd.randrange(p) for _ in range(v)]
        run = Run(lib, ctx, C, io, g, name, T, W, v)
        try:
            run.all(challenges, scribble_after=99)
        finally:
            run.close()
        N = 1 << v
        for j in sorted({1, 2, v - 1}):
            M = N >> j
            d_t, k_t = io.alloc((arity * M + 1) * 32)
            lib.mle_fix_fr_dev(ctx, C.curve_id, run.d_t, v, arity, point_bytes(challenges[:j]), j, d_t)
            d_w, k_w = (io.alloc((M + 1) * 32) if weight else (None, None))
            if weight:
                lib.mle_fix_fr_dev(ctx, C.curve_id, run.d_w, v, 1, point_bytes(challenges[:j]), j, d_w)
            with g.sumcheck_dev(name, d_t, d_w, v - j) as sc:
                assert sc.round(None) == run.bytes[j], (C.name, name, "restart after %d rounds" % j)
            assert io.read(k_t, (arity * M + 1) * 32)[arity * M * 32:] == A5
    finally:
        g.free()


# ---- contract ----------------------------------------------------------------------------------------------------------------------
def policy_case(lib, ctx, C, io, policy, v=9):
    """every value from -3 to 12 and 100 leaves every byte of a whole run and of fix / eval unchanged"""
    p = C.r
    arity, terms = predicates(C)["r1cs"]
    rnd = random.Random("sumcheck/policy/%d" % C.curve_id)
    g = load_predicates(lib, ctx, C, ("r1cs",))
    try:
        T, W = random_tables(C, rnd, arity, v, True)
        challenges = [rnd.randrange(p) for _ in range(v)]
        fb = unraw(x for t in T for x in t)
        want = None
        for value in [P_DEFAULT] + list(range(-3, 13)) + [100]:
            policy.setenv(POLICY, value)
            run = Run(lib, ctx, C, io, g, "r1cs", T, W, v)
            try:
                run.all(challenges)
            finally:
                run.close()
            got = (run.bytes, dev_fix(lib, ctx, C, io, fb, v, arity, challenges[:3]), dev_fix(lib, ctx, C, io, fb, v, arity, challenges, True))
            if want is None:
                want = got
                msgs, finals = prover_ref(p, terms, T, W, 3, challenges)
                assert run.bytes == [mont(C, m) for m in msgs] + [mont(C, finals)]
            assert got == want, (C.name, "SUMCHECK_LANE_PAIRS = %d changed the bytes" % value)
    finally:
        g.free()
        policy.setenv(POLICY, P_DEFAULT)


def interleaved_case(lib, ctx, C, io, v=5):
    """other entries on the same context between two rounds (ark355_evals_eval_fr_dev, ark355_gr1cs_quotient_dev, ark355_mle_*) change
    nothing: the state lives in the handle"""
    p = C.r
    arity, terms = predicates(C)["deg3"]
    rnd = random.Random("sumcheck/interleaved/%d" % C.curve_id)
    g = load_predicates(lib, ctx, C, ("deg3",))
    try:
        T, W = random_tables(C, rnd, arity, v, True)
        D = degree_of(terms) + 1
        challenges = [rnd.randrange(p) for _ in range(v)]
        z = qc.random_z(C, rnd, 9)
        d_z, k_z = io.to_dev(z_bytes(C, z))
        h_len = g.quotient_dims("deg3")[3]
        d_h, k_h = io.alloc(h_len * 32)
        eb = unraw(rnd.randrange(p) for _ in range(1 << 11))
        run = Run(lib, ctx, C, io, g, "deg3", T, W, v)
        try:
            msgs = []
            for j in range(v):
                msgs.append(run.round(challenges[j - 1] if j else None))
                ec.dev_eval(lib, ctx, C, io, eb, 11, 1, 0, rnd.randrange(p))
                g.quotient_dev("deg3", d_z, len(z), d_h)
                dev_fix(lib, ctx, C, io, eb, 11, 1, challenges[:3])
                dev_eq(lib, ctx, C, io, challenges[:4])
            finals = run.finish(challenges[-1])
        finally:
            run.close()
        assert (msgs, finals) == prover_ref(p, terms, T, W, D, challenges), C.name
    finally:
        g.free()


def order_case(lib, ctx, C, io):
    """calls out of order are ARK355_EINVAL with a message and leave the state usable; v = 0 takes no round"""
    p = C.r
    arity, terms = predicates(C)["sr1cs"]
    rnd = random.Random("sumcheck/order/%d" % C.curve_id)
    g = load_predicates(lib, ctx, C, ("sr1cs",))
    try:
        v = 3
        T, W = random_tables(C, rnd, arity, v, True)
        ch = [rnd.randrange(p) for _ in range(v)]
        want_msgs, want_finals = prover_ref(p, terms, T, W, 3, ch)
        run = Run(lib, ctx, C, io, g, "sr1cs", T, W, v)
        try:
            expect_refusal(lib, ctx, lambda: run.sc.round(5), needle="order")              # a challenge in round 1
            expect_refusal(lib, ctx, lambda: run.sc.finish(5), needle="order")             # finish before the rounds
            assert run.round(None) == want_msgs[0]
            expect_refusal(lib, ctx, lambda: run.sc.round(None), needle="order")           # NULL later
            expect_refusal(lib, ctx, lambda: run.sc.round(p), needle="challenge is not below r")
            expect_refusal(lib, ctx, lambda: run.sc.finish(ch[0]), needle="order")
            assert run.sc.info()[3] == 1
            assert run.round(ch[0]) == want_msgs[1] and run.round(ch[1]) == want_msgs[2]
            expect_refusal(lib, ctx, lambda: run.sc.round(ch[2]), needle="order")          # a round after the v-th
            expect_refusal(lib, ctx, lambda: run.sc.finish(None), needle="order")
            expect_refusal(lib, ctx, lambda: run.sc.finish(p), needle="challenge is not below r")
            assert run.finish(ch[2]) == want_finals
            expect_refusal(lib, ctx, lambda: run.sc.finish(ch[2]), needle="finished")
            expect_refusal(lib, ctx, lambda: run.sc.round(ch[2]), needle="finished")
            assert run.sc.info() == (3, arity, 4, 3)
        finally:
            run.close()
        for weight in (True, False):                            # v = 0: finish(NULL) returns the inputs' single entries
            T, W = random_tables(C, rnd, arity, 0, weight)
            run = Run(lib, ctx, C, io, g, "sr1cs", T, W, 0)
            try:
                expect_refusal(lib, ctx, lambda: run.sc.round(None), needle="order")
                expect_refusal(lib, ctx, lambda: run.sc.finish(7), needle="order")
                assert run.finish(None) == [t[0] for t in T] + [W[0] if W else 1]
                run.untouched()
            finally:
                run.close()
    finally:
        g.free()


def dirty_sequence(lib, ctx, C, io):
    """in a fresh context: a large run, a small eval, a small run on other data without a weight, a large fix, the large run again,
    a refusal, a good call; every step against the reference"""
    p = C.r
    rnd = random.Random("sumcheck/dirty/%d" % C.curve_id)
    g = load_predicates(lib, ctx, C, ("r1cs", "deg3"))
    try:
        big_v = 10
        T, W = random_tables(C, rnd, 3, big_v, True)
        terms = predicates(C)["r1cs"][1]
        seed = rnd.getrandbits(64)
        first = check_run(lib, ctx, C, io, g, "r1cs", terms, T, W, big_v, random.Random(seed), (C.name, "large run"))
        small = [rnd.randrange(p) for _ in range(8)]
        pt = [rnd.randrange(p) for _ in range(3)]
        assert raw(dev_fix(lib, ctx, C, io, unraw(small), 3, 1, pt, True)) == [eval_def(p, small, pt)], (C.name, "small eval")
        T2, _ = random_tables(C, rnd, 4, 2, False)
        check_run(lib, ctx, C, io, g, "deg3", predicates(C)["deg3"][1], T2, None, 2, rnd, (C.name, "small run, other data"))
        flat = [x for t in T for x in t]
        got = dev_fix(lib, ctx, C, io, unraw(flat), big_v, 3, first[2][:4])
        assert got == unraw(x for t in T for x in fix_ref(p, t, first[2][:4])), (C.name, "large fix")
        assert dev_eq(lib, ctx, C, io, first[2]) == mont(C, eq_ref(p, first[2])), (C.name, "large eq")
        expect_refusal(lib, ctx, lambda: lib.mle_eval_fr(ctx, C.curve_id, unraw(small), 3, 1, point_bytes([1, p, 2])), needle="point[1]")
        again = check_run(lib, ctx, C, io, g, "r1cs", terms, T, W, big_v, random.Random(seed), (C.name, "after the refusal"))
        assert again == first
    finally:
        g.free()


def refusals_case(lib, ctx, C):
    """every refusal a test's size reaches, host and `_dev` entry alike (a refusal touches no buffer, so host memory serves both),
    each by code and with a message, each followed by a good call on the same context"""
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    rnd = random.Random(0x5C7E + C.curve_id)
    v, count = 4, 2
    fb = unraw(rnd.randrange(p) for _ in range(count << v))
    c = np.frombuffer(fb, dtype=np.uint8).copy()
    out = np.zeros(32 * 64, dtype=np.uint8)
    point = [rnd.randrange(p) for _ in range(v)]
    pt = np.frombuffer(point_bytes(point), dtype=np.uint8).copy()
    pt_r = np.frombuffer(point_bytes(point[:2] + [p] + point[3:]), dtype=np.uint8).copy()
    pt_max = np.full(32 * v, 0xFF, dtype=np.uint8)

    def good():
        assert raw(lib.mle_eval_fr(ctx, C.curve_id, fb, v, count, point_bytes(point))) == \
            [eval_def(p, raw(fb)[k << v:(k + 1) << v], point) for k in range(count)]

    def refused(rc, needle=None, code=B.EINVAL, message=True):
        assert rc == code, rc
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg
            good()

    for fn in (d.ark355_mle_eq_fr, d.ark355_mle_eq_fr_dev):
        refused(fn(ctx, C.curve_id, v, None, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, v, ptr(pt), None), "NULL")
        refused(fn(ctx, 77, v, ptr(pt), ptr(out)), "curve")
        refused(fn(ctx, C.curve_id, v, ptr(pt_r), ptr(out)), "point[2] is not below r")
        refused(fn(ctx, C.curve_id, v, ptr(pt_max), ptr(out)), "point[0] is not below r")
        refused(fn(ctx, C.curve_id, 41, None, None), "40")
        refused(fn(ctx, C.curve_id, 40, None, None), "2^40")                               # N = 2^40 itself, before a pointer is read
        refused(fn(None, C.curve_id, v, ptr(pt), ptr(out)), message=False)
    for fn in (d.ark355_mle_fix_fr, d.ark355_mle_fix_fr_dev):
        refused(fn(ctx, C.curve_id, None, v, count, ptr(pt), 2, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, None, 2, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), 2, None), "NULL")
        refused(fn(ctx, 77, ptr(c), v, count, ptr(pt), 2, ptr(out)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), v + 1, ptr(out)), "k exceeds num_vars")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt_r), 3, ptr(out)), "point[2] is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), v, MAX_COUNT + 1, ptr(pt), 2, ptr(out)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), 2, ptr(c)), "overlap")     # in place is not offered
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), 0, vp(c.ctypes.data + 32)), "overlap")
        refused(fn(ctx, C.curve_id, None, 41, 1, None, 0, None), "40")
        refused(fn(ctx, C.curve_id, None, 30, 1024, None, 0, None), "2^40")
        refused(fn(None, C.curve_id, ptr(c), v, count, ptr(pt), 2, ptr(out)), message=False)
        assert fn(ctx, C.curve_id, None, v, 0, None, 0, None) == B.OK                      # count = 0: nothing to do
    # an accepted call works on its pointers, and these are host memory: the host entry alone
    assert d.ark355_mle_fix_fr(ctx, C.curve_id, ptr(c), v, count, ptr(pt_r), 2, ptr(out)) == B.OK   # the coordinate >= r lies beyond k
    for fn in (d.ark355_mle_eval_fr, d.ark355_mle_eval_fr_dev):
        refused(fn(ctx, C.curve_id, None, v, count, ptr(pt), ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, None, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), None), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt_r), ptr(out)), "point[2] is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), v, MAX_COUNT + 1, ptr(pt), ptr(out)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), ptr(c)), "overlap")
        refused(fn(ctx, C.curve_id, None, 41, 1, None, None), "40")
        refused(fn(ctx, C.curve_id, None, 39, 2, None, None), "2^40")
        assert fn(ctx, C.curve_id, None, v, 0, ptr(pt), None) == B.OK                      # count = 0; the point is still read
    # ---- begin
    g = load_predicates(lib, ctx, C)
    try:
        idx = g._index
        h = vp()
        begin = d.ark355_gr1cs_sumcheck_begin_dev
        refused(begin(ctx, None, 0, ptr(c), None, 1, ctypes.byref(h)), "handle is NULL")
        refused(begin(ctx, g.handle, idx["sr1cs"], None, None, 1, ctypes.byref(h)), "d_tables is NULL")
        refused(begin(ctx, g.handle, idx["sr1cs"], ptr(c), None, 1, None), "out is NULL")
        refused(begin(ctx, g.handle, len(idx), ptr(c), None, 1, ctypes.byref(h)), "predicate index out of range")
        refused(begin(ctx, g.handle, idx["sr1cs"], ptr(c), None, 41, ctypes.byref(h)), "40")
        refused(begin(ctx, g.handle, idx["sr1cs"], ptr(c), None, 39, ctypes.byref(h)), "2^40")       # 3 * 2^39
        refused(begin(ctx, g.handle, idx["arity16"], ptr(c), None, 36, ctypes.byref(h)), "2^40")     # 17 * 2^36
        refused(begin(ctx, g.handle, idx["deg32"], ptr(c), None, 1, ctypes.byref(h)), "degree as written is 32")
        refused(begin(ctx, g.handle, idx["deg31"], ptr(c), ptr(c), 1, ctypes.byref(h)), "degree as written is 31")   # 33 points with a weight
        refused(begin(ctx, g.handle, idx["deg-huge"], ptr(c), None, 1, ctypes.byref(h)), "degree as written is 8589934590")
        assert h.value is None
        assert begin(None, g.handle, idx["sr1cs"], ptr(c), None, 1, ctypes.byref(h)) == B.EINVAL
        assert d.ark355_sumcheck_info(None, None, None, None, None) == B.EINVAL
        refused(d.ark355_sumcheck_round(ctx, None, None, ptr(out)), "sumcheck handle is NULL")
        refused(d.ark355_sumcheck_finish(ctx, None, None, ptr(out)), "sumcheck handle is NULL")
        d.ark355_sumcheck_free(None)
        assert begin(ctx, g.handle, idx["deg31"], ptr(c), None, 1, ctypes.byref(h)) == B.OK and h.value     # 32 points: legal
        refused(d.ark355_sumcheck_round(ctx, h, None, None), "output is NULL")
        assert d.ark355_sumcheck_info(h, None, None, None, None) == B.OK
        d.ark355_sumcheck_free(h)
    finally:
        g.free()


# ---- [GPU only] -------------------------------------------------------------------------------------------------------------------
def large_case(lib, ctx, C, io, policy, v=20):
    """random R1CS-shaped tables with a weight at N = 2^v: the verifier chain on the library's own messages (the sum over the hypercube
    is too slow in Python and is not used), the finals against ark355_mle_eval_fr_dev, the restart equivalence at j = 1, and byte
    identity between SUMCHECK_LANE_PAIRS = 1 -- which the measurements made the default -- and 4"""
    p = C.r
    arity, terms = predicates(C)["r1cs"]
    rnd = random.Random("sumcheck/large/%d" % C.curve_id)
    N = 1 << v
    words = np.random.default_rng(0x5C + C.curve_id).integers(0, 256, size=((arity + 1) * N, 32), dtype=np.uint8)
    words[:, 31] &= (1 << ((p >> 248).bit_length() - 1)) - 1    # words below r: valid Montgomery images
    d_all, k_all = io.to_dev(words.tobytes())
    d_t, d_w = d_all, d_all + arity * N * 32
    challenges = [rnd.randrange(p) for _ in range(v)]
    g = load_predicates(lib, ctx, C, ("r1cs",))
    try:
        runs = {}
        for P in (1, P_OTHER):
            policy.setenv(POLICY, P)
            with g.sumcheck_dev("r1cs", d_t, d_w, v) as sc:
                out = [sc.round(challenges[j - 1] if j else None) for j in range(v)]
                out.append(sc.finish(challenges[-1]))
            runs[P] = out
        assert runs[1] == runs[P_OTHER], (C.name, "SUMCHECK_LANE_PAIRS = 1 (the default) against %d" % P_OTHER)
        msgs = [fr_list(C, b) for b in runs[1][:-1]]
        finals = fr_list(C, runs[1][-1])
        verify(p, terms, (msgs[0][0] + msgs[0][1]) % p, msgs, challenges, finals, (C.name, "2^%d" % v))
        d_e, k_e = io.alloc((arity + 2) * 32)
        lib.mle_eval_fr_dev(ctx, C.curve_id, d_all, v, arity + 1, point_bytes(challenges), d_e)
        got = io.read(k_e, (arity + 2) * 32)
        assert got[(arity + 1) * 32:] == A5 and got[:(arity + 1) * 32] == runs[1][-1], (C.name, "finals against mle_eval")
        d_f, k_f = io.alloc(((arity + 1) * (N // 2) + 1) * 32)
        lib.mle_fix_fr_dev(ctx, C.curve_id, d_all, v, arity + 1, point_bytes(challenges[:1]), 1, d_f)
        with g.sumcheck_dev("r1cs", d_f, d_f + arity * (N // 2) * 32, v - 1) as sc:
            assert sc.round(None) == runs[1][1], (C.name, "restart after one round")
        assert io.read(k_all, 64) == words.tobytes()[:64]
    finally:
        g.free()
        policy.setenv(POLICY, P_DEFAULT)
