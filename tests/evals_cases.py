"""Cases of the openings in the evaluation basis, shared by the CPU-emulator tier and the GPU tier (tests/test_emul_evals.py,
tests/test_gpu_evals.py): ark355_evals_eval_fr, ark355_evals_div_linear_fr, their `_dev` variants and ark355_gr1cs_mat_vec_dev
(include/ark355.h "Openings in the evaluation basis").  Every comparison is byte for byte or an exact identity of integers.

Three references for every input:
  (a) the integer formulas of the header: the barycentric sum outside the domain, e_j inside it; q_i = (e_i - y) / (a_i - x) and
      q_j = - sum_{i != j} q_i w^(i-j).  One batch inversion per (domain, x) serves every data vector (PointRef);
  (b) the coefficient route through existing entries: ark355_ntt_fr(inverse, coset) -> ark355_poly_eval_fr must give y, and
      ark355_poly_div_linear_fr -> ark355_ntt_fr(forward, coset) must give q and y;
  (c) the defining identity q_i (a_i - x) + y = e_i at every point.
Both outputs are linear in the values, so (a) and (c) work on the raw Montgomery images (v R mod r) with the canonical x and compare
the images: no conversion per element.

At the default decomposition, up to 2^FULL_CROSS_MAX_LOG points (one wave), every data pattern meets every point on both domains.
Above it, and under EVALS_LANE_POINTS = 1 and 3, every point runs on random data and every pattern at one outside and one inside
point: what a larger domain or another decomposition adds is borders of lanes, waves and workgroups, which depend on the point's
index and not on the data.

The `_dev` variants always write into buffers pre-filled with 0xA5 that are one element longer than needed, and the extra element
is checked after every call.  `io` carries the tier's device memory, as in tests/sr1cs_cases.py.  Not reachable at a test's size,
and so not covered: ARK355_ENOMEM."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import columns_cases as cc
import gr1cs_cases as gc
import poly_cases as pc
import quotient_cases as qc
import sr1cs_cases as sc
from helpers import z_bytes
from oracle import serialize as Z
from oracle.ntt import Domain
from snark_amd import _binding as B

E_DEFAULT = 8                               # EVALS_LANE_POINTS's default (snark_amd/csrc/evals_impl.cuh); a workgroup is 256 lanes
POLICY = "ARK355_EVALS_LANE_POINTS"
MAX_COUNT = 1024                            # ARK355_POLY_MAX_COUNT
A5 = b"\xA5" * 32
# one full lane (3), one wave (9), one workgroup (11), two (12: the sum kernel adds two partials), four (13)
SHAPES_DEFAULT = (0, 1, 2, 3, 4, 9, 10, 11, 12, 13)
SHAPES_E1 = (6, 8, 9)                       # one wave, one workgroup, two
SHAPES_E3 = (10,)                           # a workgroup of 768 points: borders off the powers of two
FULL_CROSS_MAX_LOG = 9
INSIDE_J = (0, -1, 7, 8, 511, 512, 2047, 2048)      # both ends, and each side of a lane, a wave and a workgroup border at E = 8

xb = pc.xb
raw = pc.raw
unraw = pc.unraw
expect_refusal = pc.expect_refusal


def two_adicity(C):
    return cc.two_adicity(C)


# ---- (a): plain integers --------------------------------------------------------------------------------------------------------------
def batch_inv(p, vals):
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % p
    inv = pow(acc, -1, p)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % p
        inv = inv * vals[i] % p
    return out


class PointRef:
    """the domain a_i = s w^i and everything about x that does not depend on the data"""

    def __init__(self, C, log_n, coset, x):
        p = self.p = C.r
        D = Domain(C, log_n)
        self.N, self.x = D.n, x % p
        self.s = D.g if coset else 1
        self.w, a = [], []
        t = 1
        for _ in range(self.N):
            self.w.append(t)
            a.append(self.s * t % p)
            t = t * D.omega % p
        self.a = a
        xs = self.x * pow(self.s, -1, p) % p
        self.inside = pow(xs, self.N, p) == 1
        self.j = a.index(self.x) if self.inside else None
        assert self.inside == (self.x in a)
        self.c = (pow(xs, self.N, p) - 1) * pow(self.N, -1, p) % p
        self.bary = None if self.inside else batch_inv(p, [(xs - wi) % p for wi in self.w])          # 1 / (x' - w^i)
        self.den = batch_inv(p, [(ai - self.x) % p if i != self.j else 1 for i, ai in enumerate(a)])  # 1 / (a_i - x)

    def eval(self, e):
        p = self.p
        if self.inside:
            return e[self.j]
        return self.c * sum(ei * wi % p * bi for ei, wi, bi in zip(e, self.w, self.bary)) % p

    def div(self, e):
        p, j = self.p, self.j
        y = self.eval(e)
        q = [(ei - y) * di % p for ei, di in zip(e, self.den)]
        if j is not None:
            q[j] = 0
            q[j] = -sum(qi * self.w[(i - j) % self.N] for i, qi in enumerate(q)) % p
        return q, y

    def check_identity(self, e, q, y, tag, indices=None):
        p = self.p
        for i in (range(self.N) if indices is None else indices):
            assert q[i] < p and (q[i] * (self.a[i] - self.x) + y) % p == e[i], (tag, "q[%d] (a_%d - x) + y != e[%d]" % (i, i, i))


# ---- the `_dev` variants behind 0xA5 ---------------------------------------------------------------------------------------------
def dev_eval(lib, ctx, C, io, eb, log_n, count, coset, x):
    d_e, k0 = io.to_dev(eb or A5)
    d_o, k1 = io.alloc((count + 1) * 32)
    lib.evals_eval_fr_dev(ctx, C.curve_id, d_e, log_n, count, coset, xb(x), d_o)
    got = io.read(k1, (count + 1) * 32)
    assert got[count * 32:] == A5, "eval wrote behind its output"
    return got[:count * 32]


def dev_div(lib, ctx, C, io, eb, log_n, count, coset, x, want_rem=True, in_place=False):
    size = (count << log_n) * 32
    d_e, k0 = io.to_dev(eb + A5)
    d_q, k1 = (d_e, k0) if in_place else io.alloc(size + 32)
    d_r, k2 = io.alloc((count + 1) * 32) if want_rem else (None, None)
    lib.evals_div_linear_fr_dev(ctx, C.curve_id, d_e, log_n, count, coset, xb(x), d_q, d_r)
    q = io.read(k1, size + 32)
    assert q[size:] == A5, "div_linear wrote behind q_out"
    if not in_place:
        assert io.read(k0, size + 32) == eb + A5, "div_linear changed its input"
    rem = None
    if want_rem:
        rem = io.read(k2, (count + 1) * 32)
        assert rem[count * 32:] == A5, "div_linear wrote behind rem_out"
        rem = rem[:count * 32]
    return q[:size], rem


# ---- (b): the coefficient route through existing entries ------------------------------------------------------------------------------
def coefficient_route(lib, ctx, C, eb, log_n, count, coset, x):
    N = 1 << log_n
    coeffs = b"".join(lib.ntt(ctx, C.curve_id, eb[32 * N * k:32 * N * (k + 1)], log_n, inverse=True, coset=bool(coset))
                      for k in range(count))
    y = lib.poly_eval_fr(ctx, C.curve_id, coeffs, N, count, xb(x))
    qc_, rem = lib.poly_div_linear_fr(ctx, C.curve_id, coeffs, N, count, xb(x))
    q = b"".join(lib.ntt(ctx, C.curve_id, qc_[32 * N * k:32 * N * (k + 1)], log_n, inverse=False, coset=bool(coset))
                 for k in range(count))
    assert rem == y
    return q, y


def check_all(lib, ctx, C, ref, eb, log_n, count, coset, x, q, y, rem, tag):
    """(a), (b) and (c) for `count` vectors"""
    N = 1 << log_n
    assert rem == y, (C.name, tag, "rem != eval")
    want_q, want_y = b"", b""
    for k in range(count):
        e = raw(eb[32 * N * k:32 * N * (k + 1)])
        qk, yk = ref.div(e)
        want_q += unraw(qk)
        want_y += unraw([yk])
        ref.check_identity(e, qk, yk, (C.name, tag, "reference"))
    assert y == want_y, (C.name, tag, "eval against the integer formula")
    assert q == want_q, (C.name, tag, "div_linear against the integer formulas", qc.first_difference(q, want_q))
    for k in range(count):                                     # (c) on the bytes the library returned
        ref.check_identity(raw(eb[32 * N * k:32 * N * (k + 1)]), raw(q[32 * N * k:32 * N * (k + 1)]), raw(y[32 * k:32 * k + 32])[0],
                           (C.name, tag))
    rq, ry = coefficient_route(lib, ctx, C, eb, log_n, count, coset, x)
    assert y == ry, (C.name, tag, "eval against ntt -> poly_eval")
    assert q == rq, (C.name, tag, "div_linear against ntt -> poly_div_linear -> ntt", qc.first_difference(q, rq))


# ---- 1: shapes, points and data -------------------------------------------------------------------------------------------------------
def outside_points(C, rnd, log_n, coset):
    """0, 1 (outside only on the coset), r - 1 (outside H_N only for N = 1, and on the coset), 7, a random one, and g a_1 for
    coset = 0: every one is checked against the domain by PointRef, which takes the inside branch where the point lies inside"""
    D = Domain(C, log_n)
    return [0, 1, C.r - 1, 7, rnd.randrange(C.r), D.g * D.omega % C.r]


def inside_points(C, log_n, coset):
    D = Domain(C, log_n)
    s = D.g if coset else 1
    js = sorted({j % D.n for j in INSIDE_J if -1 <= j < D.n})
    return [(j, s * pow(D.omega, j, C.r) % C.r) for j in js]


def patterns(C, rnd, ref, log_n, coset):
    p, N = C.r, 1 << log_n
    out = {"zero": [0] * N, "all r-1": [p - 1] * N, "constant": [rnd.randrange(1, p)] * N, "random": [rnd.randrange(p) for _ in range(N)]}
    one = [0] * N
    one[rnd.randrange(N)] = rnd.randrange(1, p)
    out["single entry"] = one
    if N >= 2:                                                 # the values of (X - x) s(X) for deg s <= N - 2: y = 0 and q = s
        D = Domain(C, log_n)
        sv = [rnd.randrange(p) for _ in range(N - 1)] + [0]
        sv = D.coset_fft(sv) if coset else D.fft(sv)
        out["root"] = [(ai - ref.x) * si % p for ai, si in zip(ref.a, sv)]
        out["root/s"] = sv
    return out


def one_input(lib, ctx, C, io, policy, E, ref, eb, log_n, coset, x, tag):
    y = dev_eval(lib, ctx, C, io, eb, log_n, 1, coset, x)
    q, rem = dev_div(lib, ctx, C, io, eb, log_n, 1, coset, x)
    check_all(lib, ctx, C, ref, eb, log_n, 1, coset, x, q, y, rem, tag)
    if E != E_DEFAULT:
        policy.setenv(POLICY, E)
        try:
            assert dev_eval(lib, ctx, C, io, eb, log_n, 1, coset, x) == y, (C.name, tag, "EVALS_LANE_POINTS = %d changed eval" % E)
            assert dev_div(lib, ctx, C, io, eb, log_n, 1, coset, x) == (q, rem), (C.name, tag, "EVALS_LANE_POINTS = %d changed div" % E)
        finally:
            policy.setenv(POLICY, E_DEFAULT)
    return q, y


def shape_case(lib, ctx, C, io, policy, E, log_n):
    p, N = C.r, 1 << log_n
    assert lib.ctx_get_policy(ctx, "EVALS_LANE_POINTS") == E_DEFAULT
    for coset in (0, 1):
        rnd = random.Random("evals/shape/%d/%d/%d/%d" % (E, log_n, coset, C.curve_id))
        pts = [(None, x) for x in outside_points(C, rnd, log_n, coset)] + inside_points(C, log_n, coset)
        full = log_n <= FULL_CROSS_MAX_LOG and E == E_DEFAULT
        seen_inside = False
        for n_pt, (j, x) in enumerate(pts):
            ref = PointRef(C, log_n, coset, x)
            if j is not None:
                assert ref.inside and ref.j == j
                seen_inside = True
            pats = patterns(C, rnd, ref, log_n, coset)
            every = full or n_pt == 4 or (j is not None and j == pts[-1][0])
            for name, e in pats.items():
                if name == "root/s" or not (every or name == "random"):
                    continue
                tag = "%s, E = %d, log_n = %d, coset = %d, x = %d%s" % (name, E, log_n, coset, x, "" if j is None else " = a_%d" % j)
                q, y = one_input(lib, ctx, C, io, policy, E, ref, unraw(e), log_n, coset, x, tag)
                if name == "constant":
                    assert q == bytes(32 * N) and y == unraw(e[:1]), (C.name, tag)
                if name == "root":
                    assert y == bytes(32) and q == unraw(pats["root/s"]), (C.name, tag, "(X - x) s(X) / (X - x) != s")
                if name == "zero":
                    assert q == bytes(32 * N) and y == bytes(32), (C.name, tag)
        assert seen_inside


# ---- 2: several vectors in one call ---------------------------------------------------------------------------------------------------
def count_case(lib, ctx, C, io, count, log_n):
    """vector k differs from the others and every output is addressed by k; the host variants give the same bytes"""
    p, N = C.r, 1 << log_n
    rnd = random.Random("evals/count/%d/%d/%d" % (count, log_n, C.curve_id))
    eb = unraw(rnd.randrange(p) for _ in range(count * N))
    D = Domain(C, log_n)
    for coset, x in ((0, rnd.randrange(p)), (1, D.g * pow(D.omega, N - 1, p) % p), (1, rnd.randrange(p))):
        tag = "count = %d, log_n = %d, coset = %d, x = %d" % (count, log_n, coset, x)
        ref = PointRef(C, log_n, coset, x)
        y = dev_eval(lib, ctx, C, io, eb, log_n, count, coset, x)
        q, rem = dev_div(lib, ctx, C, io, eb, log_n, count, coset, x)
        check_all(lib, ctx, C, ref, eb, log_n, count, coset, x, q, y, rem, tag)
        if log_n == 0:
            assert q == bytes(32 * count) and y == eb, (C.name, tag)
        assert lib.evals_eval_fr(ctx, C.curve_id, eb, log_n, count, coset, xb(x)) == y, (C.name, tag, "host eval")
        assert lib.evals_div_linear_fr(ctx, C.curve_id, eb, log_n, count, coset, xb(x)) == (q, rem), (C.name, tag, "host div_linear")
        assert lib.evals_div_linear_fr(ctx, C.curve_id, eb, log_n, count, coset, xb(x), want_rem=False) == (q, None)
        q2, none = dev_div(lib, ctx, C, io, eb, log_n, count, coset, x, want_rem=False)
        assert q2 == q and none is None


# ---- 3: in place, and the overlaps that are refused ----------------------------------------------------------------------------------
def in_place_case(lib, ctx, C, io, log_n=11, count=3):
    p, N = C.r, 1 << log_n
    rnd = random.Random("evals/inplace/%d" % C.curve_id)
    eb = unraw(rnd.randrange(p) for _ in range(count * N))
    D = Domain(C, log_n)
    for coset, x in ((0, rnd.randrange(p)), (0, pow(D.omega, 1025, p))):
        ref = PointRef(C, log_n, coset, x)
        q, rem = dev_div(lib, ctx, C, io, eb, log_n, count, coset, x)
        check_all(lib, ctx, C, ref, eb, log_n, count, coset, x, q, rem, rem, "out of place")
        assert dev_div(lib, ctx, C, io, eb, log_n, count, coset, x, in_place=True) == (q, rem), (C.name, "div_linear in place", x)
    # every other overlap: one buffer of three times the size, the input in its middle third
    size = count * N * 32
    d_b, keep = io.to_dev(A5 * (count * N) + eb + A5 * (count * N))
    d_e = d_b + size
    xbytes = xb(x)
    for d_q in (d_e + 32, d_e - 32, d_e + size - 32, d_e - size + 32):
        expect_refusal(lib, ctx, lambda: lib.evals_div_linear_fr_dev(ctx, C.curve_id, d_e, log_n, count, 0, xbytes, d_q, None), needle="overlap")
    for d_r in (d_e, d_e + size - 32, d_b + 32):               # the remainder inside the input, and inside q_out = d_b
        expect_refusal(lib, ctx, lambda: lib.evals_div_linear_fr_dev(ctx, C.curve_id, d_e, log_n, count, 0, xbytes, d_b, d_r), needle="overlap")
    for d_o in (d_e, d_e + 64, d_e + size - 32, d_e - count * 32 + 32):
        expect_refusal(lib, ctx, lambda: lib.evals_eval_fr_dev(ctx, C.curve_id, d_e, log_n, count, 0, xbytes, d_o), needle="overlap")
    assert io.read(keep, 3 * size) == A5 * (count * N) + eb + A5 * (count * N), "a refused call wrote"
    assert dev_div(lib, ctx, C, io, eb, log_n, count, coset, x) == (q, rem)                # the context works afterwards


# ---- 4: the policy's edge values ---------------------------------------------------------------------------------------------------
def policy_case(lib, ctx, C, io, policy, log_n=11):
    """every value from -3 to 100 leaves every byte unchanged: outside the domain, and inside it in the second workgroup of E = 3"""
    p = C.r
    rnd = random.Random("evals/policy/%d" % C.curve_id)
    eb = unraw(rnd.randrange(p) for _ in range(1 << log_n))
    D = Domain(C, log_n)
    xs = (rnd.randrange(p), D.g * pow(D.omega, 769, p) % p)
    want = [dev_div(lib, ctx, C, io, eb, log_n, 1, 1, x) for x in xs]
    for x, (q, rem) in zip(xs, want):
        check_all(lib, ctx, C, PointRef(C, log_n, 1, x), eb, log_n, 1, 1, x, q, rem, rem, "default")
    for value in range(-3, 101):
        policy.setenv(POLICY, value)
        for x, w in zip(xs, want):
            assert dev_div(lib, ctx, C, io, eb, log_n, 1, 1, x) == w, (C.name, "EVALS_LANE_POINTS = %d changed the bytes" % value)
            assert dev_eval(lib, ctx, C, io, eb, log_n, 1, 1, x) == w[1]
    policy.setenv(POLICY, E_DEFAULT)


# ---- 5: ark355_gr1cs_mat_vec_dev --------------------------------------------------------------------------------------------------------
def mat_vec_dev(g, io, label, d_z, z_len, n, log_n=0):
    """the t x N values behind 0xA5, split per matrix; rows n .. N-1 must have been written as zero over the poison"""
    arity = g.predicates[g._index[label]].arity
    N = 1 << g.quotient_dims(label, log_n)[1]
    d_o, keep = io.alloc((arity * N + 1) * 32)
    g.mat_vec_dev(label, d_z, z_len, d_o, log_n)
    got = io.read(keep, (arity * N + 1) * 32)
    assert got[arity * N * 32:] == A5, "mat_vec_dev wrote behind its output"
    vecs = [got[k * N * 32:(k + 1) * N * 32] for k in range(arity)]
    for v in vecs:
        assert v[n * 32:] == bytes((N - n) * 32), "rows n .. N-1 are not zero"
    return d_o, keep, N, vecs


def mat_vec_system_case(lib, ctx, C, io, g, label, zb, z_len, n):
    """rows < n equal ark355_gr1cs_mat_vec; log_n = 0 and an explicit larger log_n; every refusal is followed by a good call"""
    d_z, k0 = io.to_dev(zb)
    host = g.mat_vec(label, zb)
    log0 = g.quotient_dims(label)[1]
    for log_n in (0, log0 + 2):
        _, _, N, vecs = mat_vec_dev(g, io, label, d_z, z_len, n, log_n)
        assert N == 1 << (log_n or log0) and N >= max(n, 2)
        assert [v[:n * 32] for v in vecs] == host, (C.name, label, "rows < n against ark355_gr1cs_mat_vec")
    d, vp, i = lib.dll, ctypes.c_void_p, g._index[label]
    d_o, k1 = io.alloc(len(host) * (4 << log0) * 32)
    fn = d.ark355_gr1cs_mat_vec_dev

    def refused(rc, code=B.EINVAL):
        assert rc == code and d.ark355_last_error(ctx), rc
        _, _, _, again = mat_vec_dev(g, io, label, d_z, z_len, n)
        assert [v[:n * 32] for v in again] == host

    refused(fn(ctx, None, i, vp(d_z), z_len, 0, vp(d_o)))
    refused(fn(ctx, g.handle, len(g.predicates), vp(d_z), z_len, 0, vp(d_o)))
    refused(fn(ctx, g.handle, i, None, z_len, 0, vp(d_o)))
    refused(fn(ctx, g.handle, i, vp(d_z), z_len, 0, None))
    refused(fn(ctx, g.handle, i, vp(d_z), z_len - 1, 0, vp(d_o)), B.E_ASSIGNMENT_MISSING)
    if n > 2:
        refused(fn(ctx, g.handle, i, vp(d_z), z_len, 1, vp(d_o)))                         # 2^1 < n
    refused(fn(ctx, g.handle, i, vp(d_z), z_len, two_adicity(C) + 1, vp(d_o)), B.E_POLY_DEGREE_TOO_LARGE)
    assert fn(None, g.handle, i, vp(d_z), z_len, 0, vp(d_o)) == B.EINVAL
    assert io.read(k1, 64) == A5 * 2, "a refused call wrote"


def mat_vec_case(lib, ctx, C, io, name):
    if name == "sr1cs":
        A, Bm, Cm, z, ell = sc.handmade_instance(C)
        s, _ = sc.build(lib, ctx, C, A, Bm, Cm, ell, len(z))
        try:
            n_ell, n_w, rows, _ = s.dims
            mp = n_ell + n_w
            d_z, k0 = io.to_dev(z_bytes(C, z))
            d_zp, k1 = io.alloc(mp * 32)
            s.assignment_dev(d_z, len(z), d_zp)
            mat_vec_system_case(lib, ctx, C, io, s.system, sc.SR1CS_LABEL, io.read(k1, mp * 32), mp, rows)
        finally:
            s.free()
        return
    ell, w, spec, z = cc.qap_systems(C)[name]
    g = gc.load(lib, ctx, C, ell, w, spec)
    try:
        label = next(iter(spec))
        mat_vec_system_case(lib, ctx, C, io, g, label, z_bytes(C, z), len(z), len(spec[label][2][0]))
    finally:
        g.free()


# ---- 6: the chain on device pointers, KZG over a Lagrange-basis key ---------------------------------------------------------------------
def chain_on(lib, ctx, C, io, g, label, terms, d_z, zb, z_len, n, seed, pairing):
    """mat_vec_dev -> evals_eval_fr_dev / evals_div_linear_fr_dev -> msm_dev over [L_i(tau)] G, device pointers throughout.
    X^N - 1 divides P(m_0, ..) only for an assignment that satisfies every row: then x is random in the whole field.  Otherwise h is
    defined by the coset g H_{DN} alone and x is a random point of it (columns_cases.qap_tau): outside H_N either way."""
    p = C.r
    rnd = random.Random(seed)
    cid = C.curve_id
    d_m, k_m, N, vecs = mat_vec_dev(g, io, label, d_z, z_len, n)
    log_n, t = N.bit_length() - 1, len(vecs)
    dims = g.quotient_dims(label)
    x, tau = cc.qap_tau(C, rnd, dims[1] + dims[2], g.which_is_unsatisfied(zb) is None), rnd.randrange(2, p)
    # m_k(x): the evaluation basis against the coefficient basis, both on device pointers
    d_y, k_y = io.alloc((t + 1) * 32)
    lib.evals_eval_fr_dev(ctx, cid, d_m, log_n, t, 0, xb(x), d_y)
    yb = io.read(k_y, (t + 1) * 32)
    assert yb[t * 32:] == A5
    d_c, k_c = io.to_dev(b"".join(vecs))
    d_s, k_s = io.alloc(N * 32)
    for k in range(t):
        lib.ntt_dev(ctx, cid, d_c + k * N * 32, d_s, log_n, inverse=True)
    d_y2, k_y2 = io.alloc(t * 32)
    lib.poly_eval_fr_dev(ctx, cid, d_c, N, t, xb(x), d_y2)
    assert io.read(k_y2, t * 32) == yb[:t * 32], (C.name, "m_k(x): evaluation basis against coefficient basis")
    # P(m_0(x), ..) = h(x) (x^N - 1)
    h_len = g.quotient_dims(label)[3]
    d_h, k_h = io.alloc(h_len * 32)
    g.quotient_dev(label, d_z, z_len, d_h)
    d_hx, k_hx = io.alloc(32)
    lib.poly_eval_fr_dev(ctx, cid, d_h, h_len, 1, xb(x), d_hx)
    mx = qc.fr_list(C, yb[:t * 32])
    hx = Z.fr_from_mont(C, io.read(k_hx, 32))
    assert gc.residual(p, terms, mx) == hx * (pow(x, N, p) - 1) % p, (C.name, "P(m(x)) != h(x) (x^N - 1)")
    # the Lagrange-basis key, built without the host seeing a scalar
    size = lib.sizes(cid)["g1"]
    G = Z.g1_raw(C, C.g1_gen)
    d_L, k_L = io.alloc(N * 32)
    lib.lagrange_fr_dev(ctx, cid, log_n, xb(tau), d_L)
    bases = lib.bases_load(ctx, cid, 1, lib.fixed_base_mul_dev(ctx, cid, 1, G, d_L, N, 1, size), N)
    commit_of = lambda v: lib.fixed_base_mul(ctx, cid, 1, G, Z.fr_canon(C, v % p), 1, size)          # noqa: E731
    try:
        e = qc.fr_list(C, vecs[0])
        p_tau = PointRef(C, log_n, 0, tau).eval(e)
        y = mx[0]
        assert lib.msm_dev(ctx, bases, d_m, N, 1, size) == commit_of(p_tau), (C.name, "the commitment of the evaluations")
        d_q, k_q = io.alloc((N + 1) * 32)
        d_r, k_r = io.alloc(64)
        lib.evals_div_linear_fr_dev(ctx, cid, d_m, log_n, 1, 0, xb(x), d_q, d_r)
        assert io.read(k_q, (N + 1) * 32)[N * 32:] == A5 and io.read(k_r, 64) == yb[:32] + A5
        com_q = lib.msm_dev(ctx, bases, d_q, N, 1, size)
        assert com_q == commit_of((p_tau - y) * pow((tau - x) % p, -1, p)), (C.name, "the commitment of the witness polynomial")
        if pairing:                                            # e([p(tau) - y] G, H) e([q(tau)] G, [-(tau - x)] H) = 1, not for y + 1
            g2 = lib.sizes(cid)["g2"]
            H = Z.g2_raw(C, C.g2_gen)
            H2 = lib.fixed_base_mul(ctx, cid, 2, H, Z.fr_canon(C, (p - (tau - x)) % p), 1, g2)
            for shift, want_one in ((0, True), (1, False)):
                d_v, k_v = io.to_dev(qc.mont(C, [(v - y - shift) % p for v in e]))           # sum_i L_i(tau) = 1
                gt, is_one = lib.multi_pairing(ctx, cid, lib.msm_dev(ctx, bases, d_v, N, 1, size) + com_q, H + H2, 2, want_gt=False)
                assert is_one == want_one, (C.name, "pairing check with y + %d" % shift)
    finally:
        lib.dll.ark355_bases_free(bases)


def chain_case(lib, ctx, C, io, name, pairing=False):
    ell, w, spec, z = cc.qap_systems(C)[name]
    g = gc.load(lib, ctx, C, ell, w, spec)
    try:
        label = next(iter(spec))
        d_z, k0 = io.to_dev(z_bytes(C, z))
        chain_on(lib, ctx, C, io, g, label, spec[label][1], d_z, z_bytes(C, z), len(z), len(spec[label][2][0]),
                 "evals/chain/%s/%d" % (name, C.curve_id), pairing)
    finally:
        g.free()


def chain_sr1cs_case(lib, ctx, C, io, A, Bm, Cm, z, ell, pairing=False):
    m = len(z)
    s, _ = sc.build(lib, ctx, C, A, Bm, Cm, ell, m)
    try:
        n_ell, n_w, rows, _ = s.dims
        mp = n_ell + n_w
        d_z, k0 = io.to_dev(z_bytes(C, z))
        d_zp, k1 = io.alloc(mp * 32)
        s.assignment_dev(d_z, m, d_zp)
        chain_on(lib, ctx, C, io, s.system, sc.SR1CS_LABEL, gc.sr1cs_terms(C.r), d_zp, io.read(k1, mp * 32), mp, rows,
                 "evals/chain/sr1cs/%d" % C.curve_id, pairing)
    finally:
        s.free()


# ---- 7: dirty scratch ----------------------------------------------------------------------------------------------------------------
def dirty_sequence(lib, ctx, C, io):
    """in a fresh context: a large div_linear, a small eval, a small div_linear on other data at a point INSIDE the domain, the large
    vectors again through eval, a refusal, a good call; every step against the references"""
    p = C.r
    rnd = random.Random("evals/dirty/%d" % C.curve_id)
    big_log, count = 13, 3
    big = unraw(rnd.randrange(p) for _ in range(count << big_log))
    x = rnd.randrange(p)
    ref = PointRef(C, big_log, 1, x)
    q, rem = dev_div(lib, ctx, C, io, big, big_log, count, 1, x)
    check_all(lib, ctx, C, ref, big, big_log, count, 1, x, q, rem, rem, "large div_linear")
    small = unraw(rnd.randrange(p) for _ in range(8))
    x2 = rnd.randrange(p)
    y2 = dev_eval(lib, ctx, C, io, small, 3, 1, 0, x2)
    assert y2 == unraw([PointRef(C, 3, 0, x2).eval(raw(small))]), (C.name, "small eval")
    other = unraw(rnd.randrange(p) for _ in range(2 * 16))
    x3 = pow(Domain(C, 4).omega, 9, p)
    q3, rem3 = dev_div(lib, ctx, C, io, other, 4, 2, 0, x3)
    check_all(lib, ctx, C, PointRef(C, 4, 0, x3), other, 4, 2, 0, x3, q3, rem3, rem3, "small div_linear inside the domain, other data")
    assert dev_eval(lib, ctx, C, io, big, big_log, count, 1, x) == rem, (C.name, "large eval")
    expect_refusal(lib, ctx, lambda: lib.evals_eval_fr(ctx, C.curve_id, small, 3, 1, 0, xb(p)), needle="x")          # x = r
    assert dev_div(lib, ctx, C, io, big, big_log, count, 1, x) == (q, rem), (C.name, "after the refusal")


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------------
def refusals_case(lib, ctx, C):
    """every refusal a test's size reaches, host and `_dev` entry alike (a refusal touches no buffer, so host memory serves both),
    each with a message, and a good call on the same context afterwards"""
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    rnd = random.Random(0xE7A1 + C.curve_id)
    log_n, count = 4, 2
    eb = unraw(rnd.randrange(p) for _ in range(count << log_n))
    c = np.frombuffer(eb, dtype=np.uint8).copy()
    out = np.zeros(32 * 64, dtype=np.uint8)
    rem = np.zeros(32 * 4, dtype=np.uint8)
    x = np.frombuffer(xb(rnd.randrange(p)), dtype=np.uint8).copy()
    x_r = np.frombuffer(xb(p), dtype=np.uint8).copy()
    x_max = np.full(32, 0xFF, dtype=np.uint8)
    too_large = two_adicity(C) + 1

    def refused(rc, needle=None, code=B.EINVAL, message=True):
        assert rc == code, rc
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg

    good = lib.evals_div_linear_fr(ctx, C.curve_id, eb, log_n, count, 1, x.tobytes())
    for fn in (d.ark355_evals_eval_fr, d.ark355_evals_eval_fr_dev):
        refused(fn(ctx, C.curve_id, None, log_n, count, 0, ptr(x), ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, None, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), None), "NULL")
        refused(fn(ctx, 77, ptr(c), log_n, count, 0, ptr(x), ptr(out)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x_r), ptr(out)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 1, ptr(x_max), ptr(out)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, MAX_COUNT + 1, 0, ptr(x), ptr(out)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), ptr(c)), "overlap")
        if too_large + 9 >= 40:                                # 2^40 elements lie within reach of MAX_COUNT on BLS12-381 (2^32) alone
            refused(fn(ctx, C.curve_id, None, too_large - 1, 1 << (41 - too_large), 0, None, None), "2^40")   # before a pointer is read
        refused(fn(ctx, C.curve_id, None, too_large, 1, 0, None, None), "radix-2", B.E_POLY_DEGREE_TOO_LARGE)
        refused(fn(ctx, C.curve_id, None, 200, 1, 0, None, None), "radix-2", B.E_POLY_DEGREE_TOO_LARGE)
        refused(fn(None, C.curve_id, ptr(c), log_n, count, 0, ptr(x), ptr(out)), message=False)
    for fn in (d.ark355_evals_div_linear_fr, d.ark355_evals_div_linear_fr_dev):
        refused(fn(ctx, C.curve_id, None, log_n, count, 0, ptr(x), ptr(out), ptr(rem)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, None, ptr(out), ptr(rem)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), None, ptr(rem)), "NULL")
        refused(fn(ctx, 77, ptr(c), log_n, count, 0, ptr(x), ptr(out), ptr(rem)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x_r), ptr(out), ptr(rem)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, MAX_COUNT + 1, 0, ptr(x), ptr(out), ptr(rem)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), vp(c.ctypes.data + 32), ptr(rem)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), ptr(out), ptr(c)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), log_n, count, 0, ptr(x), ptr(out), vp(out.ctypes.data + 32)), "overlap")
        if too_large + 9 >= 40:
            refused(fn(ctx, C.curve_id, None, too_large - 1, 1 << (41 - too_large), 0, None, None, None), "2^40")
        refused(fn(ctx, C.curve_id, None, too_large, 1, 0, None, None, None), "radix-2", B.E_POLY_DEGREE_TOO_LARGE)
        refused(fn(None, C.curve_id, ptr(c), log_n, count, 0, ptr(x), ptr(out), ptr(rem)), message=False)
    assert c.tobytes() == eb and not out.any() and not rem.any(), "a refused call wrote"
    # count = 0: ARK355_OK and nothing written
    out[:] = 0xA5
    assert d.ark355_evals_eval_fr(ctx, C.curve_id, None, log_n, 0, 0, ptr(x), None) == B.OK
    assert d.ark355_evals_div_linear_fr(ctx, C.curve_id, None, log_n, 0, 0, ptr(x), None, None) == B.OK
    assert d.ark355_evals_eval_fr_dev(ctx, C.curve_id, ptr(c), log_n, 0, 0, ptr(x), ptr(out)) == B.OK and (out == 0xA5).all()
    assert d.ark355_evals_div_linear_fr_dev(ctx, C.curve_id, ptr(c), log_n, 0, 1, ptr(x), ptr(out), ptr(out)) == B.OK and (out == 0xA5).all()
    # the context stays usable
    assert lib.evals_div_linear_fr(ctx, C.curve_id, eb, log_n, count, 1, x.tobytes()) == good
    xi = int.from_bytes(x.tobytes(), "little")
    check_all(lib, ctx, C, PointRef(C, log_n, 1, xi), eb, log_n, count, 1, xi, good[0], good[1], good[1], "after the refusals")


# ---- 9: large domains against the coefficient route on the device (GPU tier) -------------------------------------------------------------
def random_words(C, n, seed):
    """random 32-byte words with the top byte masked below r's: valid Montgomery images"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    words[:, 31] &= (1 << ((C.r >> 248).bit_length() - 1)) - 1
    return words.tobytes()


def large_case(lib, ctx, C, io, policy, log_n, E_other, j_frac=None, samples=4096):
    """one vector of 2^log_n values, x outside the domain and x = a_j: q and y byte-identical to ntt -> poly_eval / poly_div_linear
    -> ntt on device pointers, identity (c) at `samples` random indices, and EVALS_LANE_POINTS = E_other against the default"""
    p, N, cid = C.r, 1 << log_n, C.curve_id
    rnd = random.Random("evals/large/%d/%d" % (log_n, cid))
    eb = random_words(C, N, 0xE7A1 + log_n + cid)
    D = Domain(C, log_n)
    j = N - 1 - rnd.randrange(256) if j_frac is None else int(N * j_frac)
    d_e, k_e = io.to_dev(eb)
    d_c, k_c = io.to_dev(eb)
    d_s, k_s = io.alloc(N * 32)
    lib.ntt_dev(ctx, cid, d_c, d_s, log_n, inverse=True)                       # the coefficients, once
    at = lambda b, i: int.from_bytes(b[32 * i:32 * i + 32], "little")          # noqa: E731
    for x in (rnd.randrange(p), pow(D.omega, j, p)):
        d_q, k_q = io.alloc((N + 1) * 32)
        d_r, k_r = io.alloc(64)
        d_y, k_y = io.alloc(64)
        lib.evals_div_linear_fr_dev(ctx, cid, d_e, log_n, 1, 0, xb(x), d_q, d_r)
        lib.evals_eval_fr_dev(ctx, cid, d_e, log_n, 1, 0, xb(x), d_y)
        q, r = io.read(k_q, (N + 1) * 32), io.read(k_r, 64)
        assert q[N * 32:] == A5 and r[32:] == A5 and io.read(k_y, 64) == r
        # the coefficient route on device pointers
        d_w, k_w = io.alloc(N * 32)
        d_wr, k_wr = io.alloc(32)
        lib.poly_div_linear_fr_dev(ctx, cid, d_c, N, 1, xb(x), d_w, d_wr)
        lib.ntt_dev(ctx, cid, d_w, d_s, log_n, inverse=False)
        lib.poly_eval_fr_dev(ctx, cid, d_c, N, 1, xb(x), d_y)                  # also waits for the transform
        assert io.read(k_y, 32) == r[:32] and io.read(k_wr, 32) == r[:32], (C.name, log_n, "y against the coefficient route")
        want = io.read(k_w, N * 32)
        assert q[:N * 32] == want, (C.name, log_n, "q against the coefficient route", qc.first_difference(q[:N * 32], want))
        y = at(r, 0)
        idx = {rnd.randrange(N) for _ in range(samples)} | {0, N - 1, j, (j + 1) % N, j - 1}
        for i in sorted(idx):
            assert (at(q, i) * (pow(D.omega, i, p) - x) + y) % p == at(eb, i), (C.name, log_n, "identity at %d" % i)
        policy.setenv(POLICY, E_other)
        try:
            d_q2, k_q2 = io.alloc((N + 1) * 32)
            lib.evals_div_linear_fr_dev(ctx, cid, d_e, log_n, 1, 0, xb(x), d_q2, d_r)
            assert io.read(k_q2, (N + 1) * 32) == q and io.read(k_r, 64) == r, (C.name, log_n, "EVALS_LANE_POINTS = %d" % E_other)
        finally:
            policy.setenv(POLICY, E_DEFAULT)
