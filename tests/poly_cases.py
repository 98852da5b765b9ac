"""Polynomial-opening cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_poly.py, tests/test_gpu_poly.py):
ark355_poly_eval_fr, ark355_poly_div_linear_fr, ark355_poly_lincomb_fr and their `_dev` variants (include/ark355.h "Polynomial
openings") against plain Python integers and oracle.fields.  Every comparison is byte for byte or an exact identity of integers.

  eval    Horner's rule;
  div     the local recurrence q[len-1] = 0, q[j-1] = c_j + x q_j for every j, rem = c_0 + x q_0: it determines q and rem
          uniquely at one multiplication per coefficient; rem against eval byte for byte;
  lincomb Python sums.
All three are linear in the coefficients, so the references work on the raw Montgomery images (v R mod r) with the canonical x
and compare the images: no conversion per element.

The `_dev` variants always write into buffers pre-filled with 0xA5 that are one element longer than needed, and the extra
element is checked after every call.  `io` carries the tier's device memory, as in tests/sr1cs_cases.py.

The refusals of len >= 2^32 and of count * len >= 2^40 are made before any pointer is read, so they are covered with the small
buffers of the other refusals.  Not reachable at a test's size, and so not covered: ARK355_ENOMEM."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import columns_cases as cc
import gr1cs_cases as gc
import quotient_cases as qc
import sr1cs_cases as sc
from helpers import z_bytes
from oracle import serialize as Z
from oracle.ntt import Domain
from snark_amd import _binding as B

E_DEFAULT = 8                               # POLY_LANE_COEFFS's default (snark_amd/csrc/poly_impl.cuh); a workgroup is 256 lanes
MAX_COUNT = 1024                            # ARK355_POLY_MAX_COUNT
A5 = b"\xA5" * 32

# the smallest shapes at which each level of the decomposition can go wrong: a lane, a wave, a chunk, three chunks
SHAPES_DEFAULT = (0, 1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097)
SHAPES_E1 = (255, 256, 257, 513)            # chunk 256: one chunk, two, three
SHAPES_E1_GPU = (65535, 65536, 65537)       # 256^2 + 1: a third level holding one coefficient
SHAPES_E3 = (769, 1537)                     # chunk 768: borders off the powers of two
FULL_CROSS_MAX = 4097                       # above it: every point on random coefficients, every pattern at a random point


def xb(x):
    return int(x).to_bytes(32, "little")


def raw(b):
    return qc.raw_list(b)


def unraw(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def mont(C, ints):
    return qc.mont(C, ints)


# ---- references ------------------------------------------------------------------------------------------------------------------
def horner(p, c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % p
    return acc


def check_eval(C, cb, n, count, x, got, tag):
    p = C.r
    assert len(got) == 32 * count, tag
    for k in range(count):
        want = horner(p, raw(cb[32 * k * n:32 * (k + 1) * n]), x)
        assert got[32 * k:32 * (k + 1)] == want.to_bytes(32, "little"), (C.name, tag, "eval of polynomial %d" % k)


def check_div(C, cb, n, count, x, q, rem, tag, indices=None):
    """the recurrence at every j (or at `indices`); rem may be None"""
    p = C.r
    assert len(q) == 32 * count * n, tag
    for k in range(count):
        c, s = raw(cb[32 * k * n:32 * (k + 1) * n]), raw(q[32 * k * n:32 * (k + 1) * n])
        if n:
            assert s[n - 1] == 0, (C.name, tag, "polynomial %d: the top quotient coefficient is not zero" % k)
        for j in (range(1, n) if indices is None else indices):
            assert max(s[j], s[j - 1]) < p and s[j - 1] == (c[j] + x * s[j]) % p, (C.name, tag, "polynomial %d, q[%d]" % (k, j - 1))
        if rem is not None:
            want = (c[0] + x * s[0]) % p if n else 0
            assert rem[32 * k:32 * (k + 1)] == want.to_bytes(32, "little"), (C.name, tag, "remainder of polynomial %d" % k)


# ---- the `_dev` variants behind 0xA5 ---------------------------------------------------------------------------------------------
def dev_eval(lib, ctx, C, io, cb, n, count, x):
    d_c, k0 = io.to_dev(cb or A5)
    d_o, k1 = io.alloc((count + 1) * 32)
    lib.poly_eval_fr_dev(ctx, C.curve_id, d_c, n, count, xb(x), d_o)
    got = io.read(k1, (count + 1) * 32)
    assert got[count * 32:] == A5, "eval wrote behind its output"
    return got[:count * 32]


def dev_div(lib, ctx, C, io, cb, n, count, x, want_rem=True, in_place=False):
    size = count * n * 32
    d_c, k0 = io.to_dev(cb + A5)
    d_q, k1 = (d_c, k0) if in_place else io.alloc(size + 32)
    d_r, k2 = io.alloc((count + 1) * 32) if want_rem else (None, None)
    lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_c, n, count, xb(x), d_q, d_r)
    q = io.read(k1, size + 32)
    assert q[size:] == A5, "div_linear wrote behind q_out"
    if not in_place:
        assert io.read(k0, size + 32) == cb + A5, "div_linear changed its input"
    rem = None
    if want_rem:
        rem = io.read(k2, (count + 1) * 32)
        assert rem[count * 32:] == A5, "div_linear wrote behind rem_out"
        rem = rem[:count * 32]
    return q[:size], rem


def dev_lincomb(lib, ctx, C, io, pb, n, scalars, in_place=False):
    d_p, k0 = io.to_dev(pb + A5)
    d_o, k1 = (d_p, k0) if in_place else io.alloc((n + 1) * 32)
    lib.poly_lincomb_fr_dev(ctx, C.curve_id, d_p, n, len(scalars), b"".join(xb(s) for s in scalars), d_o)
    size = max(len(pb), n * 32) if in_place else n * 32
    got = io.read(k1, size + 32)
    assert got[size:] == A5, "lincomb wrote behind its output"
    if in_place:
        assert got[n * 32:size] == pb[n * 32:], "lincomb in place changed another polynomial"
    return got[:n * 32]


# ---- 1: shapes, points and coefficient patterns ------------------------------------------------------------------------------------
def points(C, rnd):
    """0, 1, r - 1, a small integer, a random one, and a 32nd root of unity: the power tables hit 1"""
    return [0, 1, C.r - 1, 7, rnd.randrange(C.r), Domain(C, 5).omega]


def patterns(C, rnd, n):
    p = C.r
    out = {"zero": [0] * n, "all r-1": [p - 1] * n, "random": [rnd.randrange(p) for _ in range(n)]}
    if n:
        out["top only"] = [0] * (n - 1) + [rnd.randrange(1, p)]
        out["c0 only"] = [rnd.randrange(1, p)] + [0] * (n - 1)
    return out


def one_input(lib, ctx, C, io, policy, E, cb, n, x, tag):
    """eval, div_linear and the remainder on one polynomial against the references; under E != 8 also the bytes of the default"""
    e0 = dev_eval(lib, ctx, C, io, cb, n, 1, x)
    q0, r0 = dev_div(lib, ctx, C, io, cb, n, 1, x)
    check_eval(C, cb, n, 1, x, e0, tag)
    check_div(C, cb, n, 1, x, q0, r0, tag)
    assert r0 == e0, (C.name, tag, "rem != eval")
    if x == 0 and n:
        assert e0 == cb[:32], (C.name, tag, "x = 0 does not give the constant coefficient")
    if E != E_DEFAULT:
        policy.setenv("ARK355_POLY_LANE_COEFFS", E)
        try:
            assert dev_eval(lib, ctx, C, io, cb, n, 1, x) == e0, (C.name, tag, "POLY_LANE_COEFFS = %d changed eval" % E)
            assert dev_div(lib, ctx, C, io, cb, n, 1, x) == (q0, r0), (C.name, tag, "POLY_LANE_COEFFS = %d changed div" % E)
        finally:
            policy.setenv("ARK355_POLY_LANE_COEFFS", E_DEFAULT)


def shape_case(lib, ctx, C, io, policy, E, n):
    p = C.r
    rnd = random.Random("poly/shape/%d/%d/%d" % (E, n, C.curve_id))
    assert lib.ctx_get_policy(ctx, "POLY_LANE_COEFFS") == E_DEFAULT
    pts, pats = points(C, rnd), patterns(C, rnd, n)
    for name, c in pats.items():
        cb = unraw(c)                                          # any word below r is a valid Montgomery image
        for x in (pts if n <= FULL_CROSS_MAX or name == "random" else pts[4:5]):
            one_input(lib, ctx, C, io, policy, E, cb, n, x, "%s, E = %d, len = %d, x = %d" % (name, E, n, x))
    if n >= 2:                                                 # x a root: p = (X - x) s(X), so rem = 0 and q = s
        x = rnd.randrange(p)
        s = [rnd.randrange(p) for _ in range(n - 1)]
        c = [(a - x * b) % p for a, b in zip([0] + s, s + [0])]
        cb = unraw(c)
        one_input(lib, ctx, C, io, policy, E, cb, n, x, "root, E = %d, len = %d" % (E, n))
        q, rem = dev_div(lib, ctx, C, io, cb, n, 1, x)
        assert rem == bytes(32) and q == unraw(s + [0]), (C.name, E, n, "(X - x) s(X) / (X - x) != s")


# ---- 2: several polynomials in one call --------------------------------------------------------------------------------------------
def count_case(lib, ctx, C, io, count, n):
    """polynomial k differs from the others and every output is addressed by k; the host variants give the same bytes"""
    p = C.r
    rnd = random.Random("poly/count/%d/%d/%d" % (count, n, C.curve_id))
    cb = unraw(rnd.randrange(p) for _ in range(count * n))
    x = rnd.randrange(p)
    tag = "count = %d, len = %d" % (count, n)
    e = dev_eval(lib, ctx, C, io, cb, n, count, x)
    q, rem = dev_div(lib, ctx, C, io, cb, n, count, x)
    check_eval(C, cb, n, count, x, e, tag)
    check_div(C, cb, n, count, x, q, rem, tag)
    assert rem == e
    if n == 0:
        assert e == bytes(32 * count)
    if n == 1:
        assert q == bytes(32 * count) and rem == cb
    assert lib.poly_eval_fr(ctx, C.curve_id, cb, n, count, xb(x)) == e, (C.name, tag, "host eval")
    assert lib.poly_div_linear_fr(ctx, C.curve_id, cb, n, count, xb(x)) == (q, rem), (C.name, tag, "host div_linear")
    assert lib.poly_div_linear_fr(ctx, C.curve_id, cb, n, count, xb(x), want_rem=False) == (q, None)
    q2, none = dev_div(lib, ctx, C, io, cb, n, count, x, want_rem=False)
    assert q2 == q and none is None


# ---- 3: in place, and the overlaps that are refused ----------------------------------------------------------------------------------
def expect_refusal(lib, ctx, fn, code=B.EINVAL, needle=None):
    try:
        fn()
    except B.Ark355Error as e:
        assert e.code == code and str(e) and (needle is None or needle in str(e)), (e.code, str(e))
        return
    raise AssertionError("the call was accepted")


def in_place_case(lib, ctx, C, io, n=2049, count=3):
    p = C.r
    rnd = random.Random("poly/inplace/%d" % C.curve_id)
    cb = unraw(rnd.randrange(p) for _ in range(count * n))
    x = rnd.randrange(p)
    q, rem = dev_div(lib, ctx, C, io, cb, n, count, x)
    check_div(C, cb, n, count, x, q, rem, "out of place")
    assert dev_div(lib, ctx, C, io, cb, n, count, x, in_place=True) == (q, rem), (C.name, "div_linear in place")
    scalars = [rnd.randrange(p) for _ in range(count)]
    out = dev_lincomb(lib, ctx, C, io, cb, n, scalars)
    assert dev_lincomb(lib, ctx, C, io, cb, n, scalars, in_place=True) == out, (C.name, "lincomb in place")
    # every other overlap: one buffer of three times the size, the input in its middle third
    size = count * n * 32
    d_b, keep = io.to_dev(A5 * (count * n) + cb + A5 * (count * n))
    d_c = d_b + size
    xbytes, sbytes = xb(x), b"".join(xb(s) for s in scalars)
    for d_q in (d_c + 32, d_c - 32, d_c + size - 32, d_c - size + 32):
        expect_refusal(lib, ctx, lambda: lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_c, n, count, xbytes, d_q, None), needle="overlap")
    for d_r in (d_c, d_c + size - 32, d_b + 32):               # the remainder inside the input, and inside q_out = d_b
        expect_refusal(lib, ctx, lambda: lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_c, n, count, xbytes, d_b, d_r), needle="overlap")
    for d_o in (d_c + 32, d_c - 32, d_c + size - 32, d_c - n * 32 + 32, d_c + n * 32):
        expect_refusal(lib, ctx, lambda: lib.poly_lincomb_fr_dev(ctx, C.curve_id, d_c, n, count, sbytes, d_o), needle="overlap")
    expect_refusal(lib, ctx, lambda: lib.poly_eval_fr_dev(ctx, C.curve_id, d_c, n, count, xbytes, d_c + 64), needle="overlap")
    assert io.read(keep, 3 * size) == A5 * (count * n) + cb + A5 * (count * n), "a refused call wrote"
    assert dev_div(lib, ctx, C, io, cb, n, count, x) == (q, rem)                # the context works afterwards


# ---- 4: lincomb ----------------------------------------------------------------------------------------------------------------------
def lincomb_case(lib, ctx, C, io, count, n):
    p = C.r
    rnd = random.Random("poly/lincomb/%d/%d/%d" % (count, n, C.curve_id))
    polys = [[rnd.randrange(p) for _ in range(n)] for _ in range(count)]
    pb = b"".join(unraw(q) for q in polys)
    choices = [[0, 1, p - 1, rnd.randrange(p)][(k + s) % 4] for s in range(4) for k in range(count)]
    for s in range(4 if count else 1):
        scalars = choices[s * count:(s + 1) * count]
        want = unraw(sum(a * q[j] for a, q in zip(scalars, polys)) % p for j in range(n))
        got = dev_lincomb(lib, ctx, C, io, pb, n, scalars)
        assert got == want, (C.name, count, n, scalars[:4], qc.first_difference(got, want))
        assert lib.poly_lincomb_fr(ctx, C.curve_id, pb, n, count, b"".join(xb(a) for a in scalars)) == want, (C.name, "host lincomb")
    if count:
        for fixed in ([0] * count, [1] * count):
            want = unraw(sum(a * q[j] for a, q in zip(fixed, polys)) % p for j in range(n))
            assert dev_lincomb(lib, ctx, C, io, pb, n, fixed) == want, (C.name, count, n, fixed[0])


# ---- 5: the chain on device pointers, KZG --------------------------------------------------------------------------------------------
class Kzg:
    """powers tau^i G of a test trapdoor as a resident base set; commitments through ark355_msm_dev on Montgomery scalars"""

    def __init__(self, lib, ctx, C, n, tau):
        self.lib, self.ctx, self.C, self.n, self.tau = lib, ctx, C, n, tau
        self.size = lib.sizes(C.curve_id)["g1"]
        self.G = Z.g1_raw(C, C.g1_gen)
        powers, t = [], 1
        for _ in range(n):
            powers.append(t)
            t = t * tau % C.r
        pts = lib.fixed_base_mul(ctx, C.curve_id, 1, self.G, b"".join(Z.fr_canon(C, v) for v in powers), n, self.size)
        self.bases = lib.bases_load(ctx, C.curve_id, 1, pts, n)

    def commit_dev(self, d_scalars, n):
        return self.lib.msm_dev(self.ctx, self.bases, d_scalars, n, 1, self.size)

    def commit_of(self, scalar):
        """[scalar] G for a scalar computed in Python"""
        return self.lib.fixed_base_mul(self.ctx, self.C.curve_id, 1, self.G, Z.fr_canon(self.C, scalar % self.C.r), 1, self.size)

    def free(self):
        self.lib.dll.ark355_bases_free(self.bases)


def kzg_on(lib, ctx, C, io, d_h, keep_h, h_len, seed, pairing):
    """d_h: h_len Montgomery Fr resident on the device (from ark355_gr1cs_quotient_dev)"""
    p = C.r
    rnd = random.Random(seed)
    tau, x, v = rnd.randrange(2, p), rnd.randrange(p), rnd.randrange(p)
    inv = pow((tau - x) % p, -1, p)
    h = qc.fr_list(C, io.read(keep_h, h_len * 32))
    h_tau = horner(p, h, tau)
    kzg = Kzg(lib, ctx, C, h_len, tau)
    try:
        # (a) eval -> div_linear -> msm, device pointers throughout
        d_y, k1 = io.alloc(64)
        d_q, k2 = io.alloc((h_len + 1) * 32)
        d_r, k3 = io.alloc(64)
        lib.poly_eval_fr_dev(ctx, C.curve_id, d_h, h_len, 1, xb(x), d_y)
        lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_h, h_len, 1, xb(x), d_q, d_r)
        yb = io.read(k1, 64)
        assert yb[32:] == A5 and io.read(k3, 64) == yb and io.read(k2, (h_len + 1) * 32)[h_len * 32:] == A5
        y = Z.fr_from_mont(C, yb[:32])
        assert y == horner(p, h, x), (C.name, "eval of h")
        com_q = kzg.commit_dev(d_q, h_len)
        assert com_q == kzg.commit_of((h_tau - y) * inv), (C.name, "the commitment of the witness polynomial")
        # (b) e([h(tau) - y] G, H) e([q(tau)] G, [-(tau - x)] H) = 1, and not for y + 1
        if pairing:
            g2 = lib.sizes(C.curve_id)["g2"]
            H = Z.g2_raw(C, C.g2_gen)
            H2 = lib.fixed_base_mul(ctx, C.curve_id, 2, H, Z.fr_canon(C, (p - (tau - x)) % p), 1, g2)
            for shift, want_one in ((0, True), (1, False)):
                d_s, k4 = io.to_dev(mont(C, [(h[0] - y - shift) % p]) + io.read(keep_h, h_len * 32)[32:])
                gt, is_one = lib.multi_pairing(ctx, C.curve_id, kzg.commit_dev(d_s, h_len) + com_q, H + H2, 2, want_gt=False)
                assert is_one == want_one, (C.name, "pairing check with y + %d" % shift)
        # folding: three polynomials with 1, v, v^2, one division, one commitment
        polys = [h] + [[rnd.randrange(p) for _ in range(h_len)] for _ in range(2)]
        scalars = [1, v, v * v % p]
        d_p, k5 = io.to_dev(mont(C, [c for q in polys for c in q]) + A5)
        d_f, k6 = io.alloc((h_len + 1) * 32)
        lib.poly_lincomb_fr_dev(ctx, C.curve_id, d_p, h_len, 3, b"".join(xb(s) for s in scalars), d_f)
        lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_f, h_len, 1, xb(x), d_f, None)           # in place
        assert io.read(k6, (h_len + 1) * 32)[h_len * 32:] == A5
        q_tau = [(horner(p, q, tau) - horner(p, q, x)) * inv % p for q in polys]                # q_k(tau), from the definition
        assert kzg.commit_dev(d_f, h_len) == kzg.commit_of(sum(s * t for s, t in zip(scalars, q_tau))), (C.name, "folded witness")
    finally:
        kzg.free()


def kzg_case(lib, ctx, C, io, name, pairing=False):
    """h of a loaded system (columns_cases.qap_systems) -> eval -> div_linear -> msm"""
    ell, w, spec, z = cc.qap_systems(C)[name]
    g = gc.load(lib, ctx, C, ell, w, spec)
    try:
        label = next(iter(spec))
        h_len = g.quotient_dims(label)[3]
        d_z, k0 = io.to_dev(z_bytes(C, z))
        d_h, k1 = io.alloc(h_len * 32)
        g.quotient_dev(label, d_z, len(z), d_h)
        kzg_on(lib, ctx, C, io, d_h, k1, h_len, "poly/kzg/%s/%d" % (name, C.curve_id), pairing)
    finally:
        g.free()


def kzg_sr1cs_case(lib, ctx, C, io, A, Bm, Cm, z, ell, pairing=False):
    """assignment -> quotient -> openings of a Square R1CS system, device pointers throughout"""
    m = len(z)
    s, _ = sc.build(lib, ctx, C, A, Bm, Cm, ell, m)
    try:
        n_ell, n_w, rows, _ = s.dims
        mp = n_ell + n_w
        h_len = s.system.quotient_dims(sc.SR1CS_LABEL)[3]
        d_z, k0 = io.to_dev(z_bytes(C, z))
        d_zp, k1 = io.alloc(mp * 32)
        d_h, k2 = io.alloc(h_len * 32)
        s.assignment_dev(d_z, m, d_zp)
        s.system.quotient_dev(sc.SR1CS_LABEL, d_zp, mp, d_h)
        kzg_on(lib, ctx, C, io, d_h, k2, h_len, "poly/kzg/sr1cs/%d" % C.curve_id, pairing)
    finally:
        s.free()


# ---- 6: the third level at the default decomposition (GPU tier) ----------------------------------------------------------------------
def third_level_case(lib, ctx, C, io, policy, n=2048 * 2048 + 1, samples=4096):
    """Random 32-byte words with the top byte masked below r's are valid Montgomery images.  What carries this test is the
    comparison of the WHOLE q and rem between POLY_LANE_COEFFS = 8 and 1 -- two independent decompositions, three levels each,
    device against device -- together with the full checks at 65 537 coefficients under POLY_LANE_COEFFS = 1.  The recurrence in
    Python is a sample: every j = -1, 0, 1 (mod 2048) below 65 536, the same residues around every multiple of 2048^2, and
    `samples` random indices."""
    p = C.r
    rng = np.random.default_rng(0x7B1D + C.curve_id)
    words = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    words[:, 31] &= (1 << ((p >> 248).bit_length() - 1)) - 1   # below the top bit of r's top byte: every word is below r
    cb = words.tobytes()
    x = random.Random(0x7B1D).randrange(p)
    d_c, k0 = io.to_dev(cb)
    d_q, k1 = io.alloc((n + 1) * 32)
    d_r, k2 = io.alloc(64)
    d_e, k3 = io.alloc(64)
    lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_c, n, 1, xb(x), d_q, d_r)
    lib.poly_eval_fr_dev(ctx, C.curve_id, d_c, n, 1, xb(x), d_e)
    q8, r8 = io.read(k1, (n + 1) * 32), io.read(k2, 64)
    assert q8[n * 32:] == A5 and r8[32:] == A5 and io.read(k3, 64) == r8
    policy.setenv("ARK355_POLY_LANE_COEFFS", 1)
    d_q1, k4 = io.alloc((n + 1) * 32)
    d_r1, k5 = io.alloc(64)
    lib.poly_div_linear_fr_dev(ctx, C.curve_id, d_c, n, 1, xb(x), d_q1, d_r1)
    assert io.read(k4, (n + 1) * 32) == q8, (C.name, qc.first_difference(io.read(k4, (n + 1) * 32), q8))
    assert io.read(k5, 64) == r8
    rnd = random.Random(0x5A3B)
    idx = {j for base in range(0, 65536 + 1, 2048) for j in (base - 1, base, base + 1)}
    idx |= {j for base in range(0, n + 1, 2048 * 2048) for j in (base - 1, base, base + 1)}
    idx |= {rnd.randrange(1, n) for _ in range(samples)}
    at = lambda b, j: int.from_bytes(b[32 * j:32 * j + 32], "little")          # noqa: E731
    assert at(q8, n - 1) == 0
    for j in sorted(j for j in idx if 1 <= j < n):
        assert at(q8, j - 1) == (at(cb, j) + x * at(q8, j)) % p, (C.name, "q[%d]" % (j - 1))
    assert at(r8, 0) == (at(cb, 0) + x * at(q8, 0)) % p


# ---- 7: dirty scratch ----------------------------------------------------------------------------------------------------------------
def dirty_sequence(lib, ctx, C, io):
    """in a fresh context: a large div_linear, a small eval, a small div_linear on other data, a lincomb, the large polynomials
    again through eval, a refusal, a good call; every step against the references"""
    p = C.r
    rnd = random.Random("poly/dirty/%d" % C.curve_id)
    n_big, count = 4097, 3
    big = unraw(rnd.randrange(p) for _ in range(count * n_big))
    x = rnd.randrange(p)
    q, rem = dev_div(lib, ctx, C, io, big, n_big, count, x)
    check_div(C, big, n_big, count, x, q, rem, "large div_linear")
    small = unraw(rnd.randrange(p) for _ in range(9))
    x2 = rnd.randrange(p)
    check_eval(C, small, 9, 1, x2, dev_eval(lib, ctx, C, io, small, 9, 1, x2), "small eval")
    other = unraw(rnd.randrange(p) for _ in range(2 * 13))
    q2, rem2 = dev_div(lib, ctx, C, io, other, 13, 2, x2)
    check_div(C, other, 13, 2, x2, q2, rem2, "small div_linear, other data")
    scalars = [rnd.randrange(p), 1]
    want = unraw((scalars[0] * a + scalars[1] * b) % p for a, b in zip(raw(other[:13 * 32]), raw(other[13 * 32:])))
    assert dev_lincomb(lib, ctx, C, io, other, 13, scalars) == want, (C.name, "lincomb")
    e = dev_eval(lib, ctx, C, io, big, n_big, count, x)
    check_eval(C, big, n_big, count, x, e, "large eval")
    assert e == rem
    expect_refusal(lib, ctx, lambda: lib.poly_eval_fr(ctx, C.curve_id, small, 9, 1, xb(p)), needle="x")          # x = r
    assert dev_div(lib, ctx, C, io, big, n_big, count, x) == (q, rem), (C.name, "after the refusal")


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------------
def refusals_case(lib, ctx, C):
    """every refusal a test's size reaches, host and `_dev` entry alike (a refusal touches no buffer, so host memory serves both),
    each with a message, and a good call on the same context afterwards"""
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    rnd = random.Random(0x2EF0 + C.curve_id)
    n, count = 13, 2
    cb = unraw(rnd.randrange(p) for _ in range(count * n))
    c = np.frombuffer(cb, dtype=np.uint8).copy()
    out = np.zeros(32 * 64, dtype=np.uint8)
    rem = np.zeros(32 * 4, dtype=np.uint8)
    x = np.frombuffer(xb(rnd.randrange(p)), dtype=np.uint8).copy()
    x_r = np.frombuffer(xb(p), dtype=np.uint8).copy()
    x_max = np.full(32, 0xFF, dtype=np.uint8)
    sc_ok = np.frombuffer(xb(3) + xb(p - 1), dtype=np.uint8).copy()
    sc_bad = np.frombuffer(xb(3) + xb(p), dtype=np.uint8).copy()

    def refused(rc, needle=None, message=True):
        assert rc == B.EINVAL, rc
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg

    good = lib.poly_div_linear_fr(ctx, C.curve_id, cb, n, count, x.tobytes())
    check_div(C, cb, n, count, int.from_bytes(x.tobytes(), "little"), good[0], good[1], "before")
    for fn in (d.ark355_poly_eval_fr, d.ark355_poly_eval_fr_dev):
        refused(fn(ctx, C.curve_id, None, n, count, ptr(x), ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, None, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x), None), "NULL")
        refused(fn(ctx, 77, ptr(c), n, count, ptr(x), ptr(out)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x_r), ptr(out)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x_max), ptr(out)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), n, MAX_COUNT + 1, ptr(x), ptr(out)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x), ptr(c)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 32, 1, ptr(x), ptr(out)), "2^32")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 30, MAX_COUNT, ptr(x), ptr(out)), "2^40")
        refused(fn(None, C.curve_id, ptr(c), n, count, ptr(x), ptr(out)), message=False)
    for fn in (d.ark355_poly_div_linear_fr, d.ark355_poly_div_linear_fr_dev):
        refused(fn(ctx, C.curve_id, None, n, count, ptr(x), ptr(out), ptr(rem)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, None, ptr(out), ptr(rem)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x), None, ptr(rem)), "NULL")
        refused(fn(ctx, 77, ptr(c), n, count, ptr(x), ptr(out), ptr(rem)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x_r), ptr(out), ptr(rem)), "x is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), n, MAX_COUNT + 1, ptr(x), ptr(out), ptr(rem)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x), vp(c.ctypes.data + 32), ptr(rem)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(x), ptr(out), ptr(c)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 32, 1, ptr(x), ptr(out), ptr(rem)), "2^32")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 30, MAX_COUNT, ptr(x), ptr(out), ptr(rem)), "2^40")
        refused(fn(None, C.curve_id, ptr(c), n, count, ptr(x), ptr(out), ptr(rem)), message=False)
    for fn in (d.ark355_poly_lincomb_fr, d.ark355_poly_lincomb_fr_dev):
        refused(fn(ctx, C.curve_id, None, n, count, ptr(sc_ok), ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, None, ptr(out)), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(sc_ok), None), "NULL")
        refused(fn(ctx, 77, ptr(c), n, count, ptr(sc_ok), ptr(out)), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(sc_bad), ptr(out)), "a scalar is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), n, MAX_COUNT + 1, ptr(sc_ok), ptr(out)), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, ptr(c), n, count, ptr(sc_ok), vp(c.ctypes.data + 32)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 32, count, ptr(sc_ok), ptr(out)), "2^32")
        refused(fn(ctx, C.curve_id, ptr(c), 1 << 30, MAX_COUNT, ptr(sc_ok), ptr(out)), "2^40")
        refused(fn(None, C.curve_id, ptr(c), n, count, ptr(sc_ok), ptr(out)), message=False)
    assert c.tobytes() == cb and not out.any() and not rem.any(), "a refused call wrote"
    # count = 0: ARK355_OK and nothing written -- lincomb writes its zeros
    out[:] = 0xA5
    assert d.ark355_poly_eval_fr(ctx, C.curve_id, None, n, 0, ptr(x), None) == B.OK
    assert d.ark355_poly_div_linear_fr(ctx, C.curve_id, None, n, 0, ptr(x), None, None) == B.OK
    assert d.ark355_poly_eval_fr(ctx, C.curve_id, ptr(c), n, 0, ptr(x), ptr(out)) == B.OK and (out == 0xA5).all()
    assert d.ark355_poly_div_linear_fr(ctx, C.curve_id, ptr(c), n, 0, ptr(x), ptr(out), ptr(out)) == B.OK and (out == 0xA5).all()
    assert d.ark355_poly_lincomb_fr(ctx, C.curve_id, None, n, 0, None, ptr(out)) == B.OK
    assert not out[:32 * n].any() and (out[32 * n:] == 0xA5).all()
    # the context stays usable
    assert lib.poly_div_linear_fr(ctx, C.curve_id, cb, n, count, x.tobytes()) == good


# ---- 9: the policy's edge values ---------------------------------------------------------------------------------------------------
def policy_case(lib, ctx, C, io, policy, n=2049 + 513):
    """<= 0 selects the default, anything above 8 is clamped to it, and every value in between gives the same bytes"""
    p = C.r
    rnd = random.Random("poly/policy/%d" % C.curve_id)
    cb = unraw(rnd.randrange(p) for _ in range(n))
    x = rnd.randrange(p)
    want = dev_div(lib, ctx, C, io, cb, n, 1, x)
    check_div(C, cb, n, 1, x, want[0], want[1], "default")
    for value in (0, -3, 100, 1, 2, 3, 4, 5, 6, 7, 8):
        policy.setenv("ARK355_POLY_LANE_COEFFS", value)
        assert dev_div(lib, ctx, C, io, cb, n, 1, x) == want, (C.name, "POLY_LANE_COEFFS = %d changed the bytes" % value)
        assert dev_eval(lib, ctx, C, io, cb, n, 1, x) == want[1]
