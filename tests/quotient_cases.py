"""Quotient-polynomial cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_quotient.py,
tests/test_gpu_quotient.py): ark355_gr1cs_quotient{,_dims,_dev} (include/ark355.h "Quotient polynomial of any predicate",
snark_amd.GR1CS.quotient*) against three references built from oracle.ntt.Domain, oracle.fields and plain integers:

  R-def  the definition: ifft of each padded M_k z over H_N, zero-extension to D N, coset_fft, the polynomial pointwise times
         ((g w_{DN}^i)^N - 1)^-1, coset_ifft -- compared byte for byte;
  R-div  no transform at all (satisfied assignments, N <= 16): the m_k interpolated with Lagrange sums, schoolbook polynomial
         arithmetic, exact division by X^N - 1 with a zero remainder;
  R-pt   one random point tau: P(m_0(tau), ..) == h(tau) (tau^N - 1), with m_k(tau) from Domain.lagrange_at and M_k z from the
         already tested ark355_gr1cs_mat_vec.
The library is never its own expected value.  `io` carries the tier's device memory, as in tests/sr1cs_cases.py."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import gr1cs_cases as gc
import lcmap_cases as lcc
import sr1cs_cases as sc
from helpers import r1cs_load_from_rows, z_bytes
from oracle import r1cs as R, serialize as Z, synthetic as S
from oracle.ntt import Domain
from snark_amd import GR1CS, LcSystem, _binding as B
from snark_amd.gr1cs import Predicate
from snark_amd.params import CURVES as PRODUCT_CURVES


# ---- plain integers ----------------------------------------------------------------------------------------------------------
def fr_list(C, b):
    return [Z.fr_from_mont(C, b[i:i + 32]) for i in range(0, len(b), 32)]


def mont(C, ints):
    return b"".join(Z.fr_mont(C, v) for v in ints)


def degree_of(terms):
    return max([sum(e for _, e in mono) for _, mono in terms], default=0)


def dims_ref(n, terms, log_n=0):
    """(degree, log_domain, log_ext, h_len) as the issue states them"""
    d = degree_of(terms)
    log_domain = log_n or max(1, (max(n, 2) - 1).bit_length())
    log_ext = 0 if d <= 2 else (d - 2).bit_length()            # D = next_pow2(d - 1)
    assert (1 << log_ext) >= max(d - 1, 1) and (log_ext == 0 or (1 << (log_ext - 1)) < d - 1)
    return d, log_domain, log_ext, 1 << (log_domain + log_ext)


def mat_vecs(C, mats, z):
    return [R.mat_vec_mul(M, z, C.r) for M in mats]


# ---- R-def ---------------------------------------------------------------------------------------------------------------------
def r_def(C, terms, mv, log_domain, log_ext):
    r = C.r
    N, L = 1 << log_domain, 1 << (log_domain + log_ext)
    dom, big = Domain(C, log_domain), Domain(C, log_domain + log_ext)
    ev = [big.coset_fft(dom.ifft(list(v) + [0] * (N - len(v))) + [0] * (L - N)) for v in mv]
    out, x = [], big.g
    for i in range(L):
        zinv = pow(pow(x, N, r) - 1, -1, r)
        out.append(gc.residual(r, terms, [e[i] for e in ev]) * zinv % r)
        x = x * big.omega % r
    return big.coset_ifft(out)


# ---- R-div -----------------------------------------------------------------------------------------------------------------------
def poly_mul(a, b, r):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % r
    return out


def poly_add(a, b, r):
    out = [0] * max(len(a), len(b))
    for i, x in enumerate(a):
        out[i] = x
    for i, y in enumerate(b):
        out[i] = (out[i] + y) % r
    return out


def interpolate(C, values, log_domain):
    """coefficients of the polynomial of degree < N through (w^i, values[i]): m(X) = 1/N sum_j X^j sum_i values[i] w^(-i j)"""
    r, N = C.r, 1 << log_domain
    wi = pow(C.root_of_unity(log_domain), -1, r)
    n_inv = pow(N, -1, r)
    vals = list(values) + [0] * (N - len(values))
    return [sum(v * pow(wi, i * j, r) for i, v in enumerate(vals)) * n_inv % r for j in range(N)]


def r_div(C, terms, mv, log_domain, h_len):
    """P(m_0, ..) / (X^N - 1) by schoolbook arithmetic; asserts the remainder is zero"""
    r, N = C.r, 1 << log_domain
    m = [interpolate(C, v, log_domain) for v in mv]
    total = []
    for coeff, mono in terms:
        t = [coeff % r]
        for var, e in mono:
            for _ in range(e):
                t = poly_mul(t, m[var], r)
        total = poly_add(total, t, r)
    total = total + [0] * max(0, N - len(total))
    q = [0] * max(0, len(total) - N)
    for i in range(len(total) - 1, N - 1, -1):                 # X^i = X^(i - N) (X^N - 1) + X^(i - N)
        q[i - N] = total[i]
        total[i - N] = (total[i - N] + total[i]) % r
    assert all(v == 0 for v in total[:N]), "X^N - 1 does not divide P(m_0, ..): the assignment is not satisfied on all N rows"
    while q and q[-1] == 0:
        q.pop()
    assert len(q) <= h_len
    return q + [0] * (h_len - len(q))


# ---- R-pt ------------------------------------------------------------------------------------------------------------------------
def raw_list(b):
    """Montgomery images as integers, unconverted: v R mod r"""
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def r_pt(C, terms, mv, log_domain, log_ext, h, seed, satisfied, montgomery=False):
    """P(m_0(tau), ..) == h(tau) (tau^N - 1) at single points, with no transform on either side.  The identity holds at EVERY
    tau only when X^N - 1 divides P(m_0, ..), that is for an assignment satisfying all N rows: then tau is drawn from the whole
    field.  For any assignment it holds on the coset g H_{DN} -- that is the definition of h -- so random points of the
    coset are checked in every case: two, or one next to the field's tau (a random tau of the field would test a remainder the
    definition does not promise when the assignment is not satisfied).  montgomery: mv and h are raw_list()s; both sums are linear
    in them, so one factor R^-1 per sum converts (2^18 conversions fewer at the large sizes)."""
    r, N = C.r, 1 << log_domain
    scale = pow(1 << 256, -1, r) if montgomery else 1
    rnd = random.Random(seed)
    big = Domain(C, log_domain + log_ext)
    taus = [big.g * pow(big.omega, rnd.randrange(big.n), r) % r for _ in range(1 if satisfied else 2)]
    if satisfied:
        taus.append(rnd.randrange(2, r))
    dom = Domain(C, log_domain)
    for tau in taus:
        lag = dom.lagrange_at(tau)
        at = [sum(l * v for l, v in zip(lag, vec)) * scale % r for vec in mv]
        h_tau = 0
        for c in reversed(h):
            h_tau = (h_tau * tau + c) % r
        h_tau = h_tau * scale % r
        assert gc.residual(r, terms, at) == h_tau * (pow(tau, N, r) - 1) % r, (C.name, "P(m(tau)) != h(tau) Z(tau)", satisfied)


# ---- systems ---------------------------------------------------------------------------------------------------------------------
def random_spec(C, rnd, label, arity, terms, n, m):
    """any matrices will do against R-def: 0-3 entries per row, coefficients of {1, -1, random}, one empty row in four"""
    p = C.r

    def row():
        return [(rnd.choice([1, p - 1, rnd.randrange(1, p)]), rnd.randrange(m)) for _ in range(rnd.choice([0, 1, 2, 3]))]
    return {label: (arity, terms, [[row() for _ in range(n)] for _ in range(arity)])}


def random_z(C, rnd, m):
    return [1] + [rnd.randrange(C.r) for _ in range(m - 1)]


def shapes(C):
    """name -> (arity, terms, n, (degree, log_domain, log_ext)): item 1 of the issue"""
    p = C.r
    deg3 = [(5, [(0, 1), (1, 1), (2, 1)]), (1, [(0, 2), (0, 1)]),            # x0 x1 x2; a repeated variable: x0^3
            (p - 7, [(1, 0), (2, 2)]), (p - 1, [(3, 1)])]                    # an x^0 factor; a constant-free linear term
    deg5 = [(1, [(0, 5)]), (3, [(0, 1), (1, 1)]), (p - 1, [(1, 1)])]
    a16 = [((p - 1) if k % 3 == 0 else k + 1, [(2 * k, 1), (2 * k + 1, 1)]) for k in range(8)] + [(2, [(15, 2)]), (9, [(4, 1)])]
    return {
        "arity1-N2": (1, [(1, [(0, 2)])], 2, (2, 1, 0)),
        "arity2-N4": (2, gc.sr1cs_terms(p), 3, (2, 2, 0)),
        "arity3-N8": (3, gc.r1cs_terms(p), 7, (2, 3, 0)),
        "arity4-deg3-N16": (4, deg3, 13, (3, 4, 1)),
        "arity4-deg3-N2": (4, deg3, 2, (3, 1, 1)),                           # D N = 4: the extended transforms below 8 points
        "arity4-deg3-N4": (4, deg3, 4, (3, 2, 1)),                           # N below 8 points, D N = 8
        "deg5-N8": (2, deg5, 5, (5, 3, 2)),
        "deg1-N4": (2, [(2, [(0, 1)]), (p - 1, [(1, 1)]), (7, [])], 4, (1, 2, 0)),
        "deg0-N4": (1, [(5, []), (0, [(0, 0)])], 3, (0, 2, 0)),
        "arity16-deg2-N8": (16, a16, 6, (2, 3, 0)),
        "arity2-n70": (2, gc.sr1cs_terms(p), 70, (2, 7, 0)),                 # a partial wave, padded rows present
        "arity4-deg3-n70": (4, deg3, 70, (3, 7, 1)),
    }


def large_shapes(C):
    """[GPU only] D N = 2^11, 2^12, 2^13 (the NTT tile is 2^11 elements: one pass and several), each with D = 1 and D = 2"""
    p = C.r
    deg3 = shapes(C)["arity4-deg3-N16"][1]
    out = {}
    for lg in (11, 12, 13):
        out["D1-2^%d" % lg] = (2, gc.sr1cs_terms(p), (1 << lg) - 5, (2, lg, 0))
        out["D2-2^%d" % lg] = (4, deg3, (1 << (lg - 1)) - 3, (3, lg - 1, 1))
    return out


class Loaded:
    """one loaded system and its label"""

    def __init__(self, lib, ctx, C, ell, w, spec):
        self.C, self.spec = C, spec
        self.g = gc.load(lib, ctx, C, ell, w, spec)
        self.label = next(iter(spec))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.g.free()

    def check_def(self, z, log_n=0, want_dims=None):
        """dims as the issue states them, the quotient equal to R-def byte for byte; returns the bytes"""
        C = self.C
        arity, terms, mats = self.spec[self.label]
        n = len(mats[0])
        dims = self.g.quotient_dims(self.label, log_n)
        assert dims == dims_ref(n, terms, log_n), (dims, dims_ref(n, terms, log_n))
        if want_dims is not None:
            assert dims[:3] == want_dims, (dims, want_dims)
        h = self.g.quotient(self.label, z, log_n)
        assert len(h) == 32 * dims[3]
        want = mont(C, r_def(C, terms, mat_vecs(C, mats, z), dims[1], dims[2]))
        assert h == want, (C.name, self.label, log_n, first_difference(h, want))
        return h


def first_difference(a, b):
    for i in range(0, min(len(a), len(b)), 32):
        if a[i:i + 32] != b[i:i + 32]:
            return "first differing element %d of %d" % (i // 32, len(a) // 32)
    return "lengths %d / %d" % (len(a), len(b))


# ---- 1: shapes against R-def -------------------------------------------------------------------------------------------------
def shape_case(lib, ctx, C, name, table=None):
    arity, terms, n, want = (table or shapes(C))[name]
    rnd = random.Random("%s/%d" % (name, C.curve_id))
    m = 9
    with Loaded(lib, ctx, C, 2, m - 2, random_spec(C, rnd, name, arity, terms, n, m)) as s:
        s.check_def(random_z(C, rnd, m), want_dims=want)


# ---- 2: policy knobs -----------------------------------------------------------------------------------------------------------
POLICIES = {"nofuse": (("NTT_NOFUSE", 1),), "rmax2": (("NTT_RMAX", 2),), "direct-fallback": (("NTT_DIRECT_MAX", 4),)}


def policy_case(lib, ctx, C, policy, which, ext, log_len=12):
    """D N = 2^12 with D = 1 (radices 2^6 x 2^6: the fused seam in the default run) and D = 2: the bytes under the knob equal the default run's,
    which equals R-def"""
    p = C.r
    rnd = random.Random("policy/%d/%d" % (ext, C.curve_id))
    if ext == 0:
        arity, terms, n = 2, gc.sr1cs_terms(p), (1 << log_len) - 9
    else:
        arity, terms, n = 4, shapes(C)["arity4-deg3-N16"][1], (1 << (log_len - 1)) - 9
    m = 9
    z = random_z(C, rnd, m)
    with Loaded(lib, ctx, C, 2, m - 2, random_spec(C, rnd, "p", arity, terms, n, m)) as s:
        default = s.check_def(z, want_dims=(2 + ext, log_len - ext, ext))
        for name, value in POLICIES[which]:
            policy.setenv("ARK355_" + name, value)
        got = s.g.quotient("p", z)
        assert got == default, (C.name, which, first_difference(got, default))


# ---- 3 + 4: satisfied systems against R-div, then one witness changed ----------------------------------------------------------
def handmade_satisfied(C):
    """the hand-made matrices of sr1cs_cases.py with an assignment that satisfies them (its own is random), solved by hand:
    row 4: z8 = 3 z3; row 3: z4 = (7 z8 + z1)^2; row 2: z5 = -z3; row 1: (2 z5 + 1) z4 = 2; row 0: (z4 + 2 z1) z6 = z5.
    With s free: z4 = s^2, z3 = (1 - 2 / s^2) / 2, z1 = s - 21 z3, z6 = z5 / (z4 + 2 z1); z2 and z7 are free."""
    p = C.r
    A, Bm, Cm, _, ell = sc.handmade_instance(C)
    rnd = random.Random(0x5A7)
    s = rnd.randrange(2, p)
    inv = lambda v: pow(v, -1, p)                              # noqa: E731
    z4 = s * s % p
    z3 = (1 - 2 * inv(z4)) * inv(2) % p
    z8, z5 = 3 * z3 % p, (p - z3) % p
    z1 = (s - 21 * z3) % p
    z6 = z5 * inv((z4 + 2 * z1) % p) % p
    z = [1, z1, rnd.randrange(p), z3, z4, z5, z6, rnd.randrange(p), z8]
    assert R.first_unsatisfied_r1cs(A, Bm, Cm, z, p) == -1
    return A, Bm, Cm, z, ell


def circuit2_satisfied(C):
    """the reference's circuit2 (gr1cs/tests/circuit2.rs:46-60) with a = 1, b = 5, c = 10: its second row a (a + b) = a + b holds
    for a = 1 only, so the a = 3 instance of sr1cs_cases.py is not satisfied"""
    cs = R.ConstraintSystem(C.r)
    R.circuit2(cs, 1, 5, 10)
    return S.cs_to_instance(cs)


def satisfied_systems(C):
    """name -> (ell, w, spec, z, column of a witness whose change breaks a row)"""
    p = C.r
    out = {}
    for name, (A, Bm, Cm, z, ell) in (("circuit2", circuit2_satisfied(C)), ("hand-made", handmade_satisfied(C))):
        assert R.first_unsatisfied_r1cs(A, Bm, Cm, z, p) == -1
        out[name] = (ell, len(z) - ell, {"R1CS": (3, gc.r1cs_terms(p), [A, Bm, Cm])}, z, len(z) - 1)
    b = gc.Builder(C, 0xDE63 + C.curve_id)
    terms = [(1, [(0, 2), (1, 1)]), (b.coeff(), [(0, 1)]), (p - 1, [(2, 1)])]        # x0^2 x1 + c x0 - x2: no constant term, so
    b.add("deg3", 3, terms, 6)                                                       # the two padded rows of N = 8 hold as well
    out["random-deg3-N8"] = (b.ell, len(b.wit), b.spec, b.z(), b.fresh["deg3"][4])
    return out


def satisfied_case(lib, ctx, C, name):
    p = C.r
    ell, w, spec, z, col = satisfied_systems(C)[name]
    with Loaded(lib, ctx, C, ell, w, spec) as s:
        arity, terms, mats = spec[s.label]
        d, log_domain, log_ext, h_len = s.g.quotient_dims(s.label)
        N = 1 << log_domain
        assert N <= 16 and s.g.which_is_unsatisfied(z) is None
        h = s.g.quotient(s.label, z)
        want = r_div(C, terms, mat_vecs(C, mats, z), log_domain, h_len)
        assert h == mont(C, want), (C.name, name, first_difference(h, mont(C, want)))
        top = h_len - ((d - 1) * N - d + 1)                    # deg h <= (d - 1) N - d
        assert top >= 1 and h[-32 * top:] == bytes(32 * top), (C.name, name, "the top coefficients are not zero")
        assert s.check_def(z) == h                             # R-def agrees with R-div
        # 4: one witness changed -- still the definition's value, and another polynomial
        zbad = list(z)
        zbad[col] = (zbad[col] + 1) % p
        assert s.g.which_is_unsatisfied(zbad) is not None
        hbad = s.check_def(zbad)
        assert hbad != h


# ---- 5: equivalence with ark355_witness_map ----------------------------------------------------------------------------------------
def witness_map_case(lib, ctx, C, n):
    """the mul-chain's A, B, C with ell rows appended (A row n + i = e_i, B and C empty): Groth16's input-consistency rows"""
    p = C.r
    A, Bm, Cm, z, ell = S.mulchain_direct(p, n)
    m = len(z)
    assert n + ell > 2
    A2 = A + [[(1, i)] for i in range(ell)]
    B2, C2 = Bm + [[] for _ in range(ell)], Cm + [[] for _ in range(ell)]
    zb = z_bytes(C, z)
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, m - ell)
    g = gc.load(lib, ctx, C, ell, m - ell, {"R1CS": (3, gc.r1cs_terms(p), [A2, B2, C2])})
    try:
        N = lib.dll.ark355_r1cs_domain_size(r1)
        assert g.quotient_dims("R1CS") == (2, N.bit_length() - 1, 0, N) and N == 1 << (n + ell - 1).bit_length()
        want = lib.witness_map(ctx, r1, zb, m, 32)
        got = g.quotient("R1CS", zb)
        assert got == want, (C.name, n, first_difference(got, want))
    finally:
        g.free()
        lib.dll.ark355_r1cs_free(r1)


def witness_map_csr_case(lib, ctx, C, ell, w, mats, z):
    """the same from CSR arrays (numpy), for sizes where row lists are slow"""
    p = C.r
    n = len(mats[0][0]) - 1
    zb = S._mont_bytes(p, z)
    one = Z.fr_mont(C, 1)
    r1 = lib.r1cs_load(ctx, C.curve_id, n, ell, w, mats)
    rp0, col0, cf0 = mats[0]
    ext = [(np.concatenate([rp0, rp0[-1] + np.arange(1, ell + 1, dtype=np.uint64)]),
            np.concatenate([col0, np.arange(ell, dtype=np.uint32)]), bytes(cf0) + one * ell)]
    for rp, col, cf in mats[1:]:
        ext.append((np.concatenate([rp, np.full(ell, rp[-1], dtype=np.uint64)]), col, cf))
    pred = Predicate("R1CS", 3, gc.r1cs_terms(p), n + ell, [e[0] for e in ext], [e[1] for e in ext], [e[2] for e in ext])
    g = GR1CS(PRODUCT_CURVES[C.curve_id], ell, w, [pred]).load(lib, ctx)
    try:
        N = lib.dll.ark355_r1cs_domain_size(r1)
        assert g.quotient_dims("R1CS")[3] == N == 1 << (n + ell - 1).bit_length()
        want = lib.witness_map(ctx, r1, zb, ell + w, 32)
        got = g.quotient("R1CS", zb)
        assert got == want, (C.name, n, first_difference(got, want))
    finally:
        g.free()
        lib.dll.ark355_r1cs_free(r1)


# ---- 6: the SR1CS chain on device pointers ---------------------------------------------------------------------------------------
def sr1cs_chain_on(lib, ctx, C, io, s, zb, m, seed, satisfied):
    """ark355_sr1cs_assignment_dev -> ark355_gr1cs_quotient_dev on ark355_sr1cs_system, device pointers throughout; satisfied:
    whether the source assignment satisfies its R1CS (then the SR1CS one satisfies every row, the zero rows included)"""
    n_ell, n_w, rows, _ = s.dims
    terms = gc.sr1cs_terms(C.r)
    d, log_domain, log_ext, h_len = s.system.quotient_dims(sc.SR1CS_LABEL)
    assert (d, log_domain, log_ext, h_len) == dims_ref(rows, terms)
    d_z, k1 = io.to_dev(zb)
    d_zp, k2 = io.alloc((n_ell + n_w) * 32)
    d_h, k3 = io.alloc(h_len * 32)
    s.assignment_dev(d_z, m, d_zp)
    s.system.quotient_dev(sc.SR1CS_LABEL, d_zp, n_ell + n_w, d_h)
    zp = io.read(k2, (n_ell + n_w) * 32)
    h = io.read(k3, h_len * 32)
    mvb = s.system.mat_vec(sc.SR1CS_LABEL, zp)
    assert (s.system.which_is_unsatisfied(zp) is None) == satisfied
    r_pt(C, terms, [raw_list(v) for v in mvb], log_domain, log_ext, raw_list(h), seed, satisfied, montgomery=True)
    if h_len < 64:
        want = mont(C, r_def(C, terms, [fr_list(C, v) for v in mvb], log_domain, log_ext))
        assert h == want, (C.name, first_difference(h, want))
    assert s.system.quotient(sc.SR1CS_LABEL, zp) == h          # the host entry takes the same route


def sr1cs_chain_case(lib, ctx, C, io, A, Bm, Cm, z, ell, seed=0x7A0):
    m = len(z)
    s, _ = sc.build(lib, ctx, C, A, Bm, Cm, ell, m)
    try:
        sr1cs_chain_on(lib, ctx, C, io, s, z_bytes(C, z), m, seed, R.first_unsatisfied_r1cs(A, Bm, Cm, z, C.r) == -1)
    finally:
        s.free()


# ---- 7: explicit log_n ---------------------------------------------------------------------------------------------------------
def explicit_log_n_case(lib, ctx, C):
    arity, terms, n, want = shapes(C)["arity4-deg3-N16"]
    rnd = random.Random(0x106 + C.curve_id)
    z = random_z(C, rnd, 9)
    with Loaded(lib, ctx, C, 2, 7, random_spec(C, rnd, "q", arity, terms, n, 9)) as s:
        h0 = s.check_def(z, want_dims=want)
        h2 = s.check_def(z, log_n=want[1] + 2, want_dims=(want[0], want[1] + 2, want[2]))
        assert len(h2) == 4 * len(h0) and h2 != h0 + bytes(3 * len(h0))      # another polynomial, not the same one padded
        assert s.check_def(z, log_n=want[1]) == h0             # the explicit form of the default


# ---- 8: a handle from ark355_gr1cs_from_lcs ----------------------------------------------------------------------------------------
def from_lcs_case(lib, ctx, C, rows=20):
    cs = lcc.bench_rs_cs(C, rows)
    system = LcSystem.from_constraint_system(C.curve_id, cs)
    g = system.finalize(lib, ctx, None)
    cs.finalize()
    z = cs.full_assignment()
    satisfied = cs.which_is_unsatisfied() is None
    try:
        label = "R1CS"
        mats = g.matrices(label)
        pred = next(q for q in g.predicates if q.label == label)
        assert pred.n == rows
        copy = GR1CS(PRODUCT_CURVES[C.curve_id], g.ell, g.w,
                     [Predicate(label, pred.arity, pred.terms, pred.n, [a for a, _, _ in mats], [b for _, b, _ in mats],
                                [c for _, _, c in mats])]).load(lib, ctx)
        try:
            assert g.quotient_dims(label) == copy.quotient_dims(label) == dims_ref(rows, gc.r1cs_terms(C.r))
            h = g.quotient(label, z)
            assert h == copy.quotient(label, z)
            mv = [fr_list(C, v) for v in copy.mat_vec(label, z)]
            r_pt(C, gc.r1cs_terms(C.r), mv, g.quotient_dims(label)[1], 0, fr_list(C, h), 0x1C5, satisfied)
        finally:
            copy.free()
    finally:
        g.free()


# ---- 9: _dims and refusals -------------------------------------------------------------------------------------------------------
def dims_and_refusals_case(lib, ctx, C):
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    two_adicity = ((p - 1) & -(p - 1)).bit_length() - 1
    assert two_adicity == {"bls12_381": 32, "bn254": 28}[C.name.lower().replace("-", "_")]
    rnd = random.Random(0x9E + C.curve_id)
    m = 9
    z = random_z(C, rnd, m)
    zb = np.frombuffer(z_bytes(C, z), dtype=np.uint8).copy()
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    out = np.zeros(32 * 64, dtype=np.uint8)

    def refused(rc, code, needle=None, message=True):
        assert rc == code, (rc, code)
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg

    def raw_dims(h, pred, log_n):
        deg, ld, le, hl = ctypes.c_uint64(77), ctypes.c_uint32(77), ctypes.c_uint32(77), ctypes.c_uint64(77)
        rc = d.ark355_gr1cs_quotient_dims(h, pred, log_n, ctypes.byref(deg), ctypes.byref(ld), ctypes.byref(le), ctypes.byref(hl))
        return rc, deg.value, ld.value, le.value, hl.value

    # the dims of every polynomial of item 1 (the quotients themselves: shape_case)
    for name, (arity, terms, n, want) in shapes(C).items():
        with Loaded(lib, ctx, C, 2, m - 2, random_spec(C, rnd, name, arity, terms, n, m)) as s:
            assert s.g.quotient_dims(name) == want + (1 << (want[1] + want[2]),) == dims_ref(n, terms), name
    # exponents summing past 2^32: the 64-bit degree is reported and refused, not wrapped
    big = [(1, [(0, 0xFFFFFFFF), (1, 0xFFFFFFFF), (0, 3)]), (p - 1, [(1, 1)])]
    with Loaded(lib, ctx, C, 2, m - 2, random_spec(C, rnd, "big", 2, big, 3, m)) as s:
        rc, deg, ld, le, hl = raw_dims(s.g.handle, 0, 0)
        assert rc == B.E_POLY_DEGREE_TOO_LARGE and deg == 2 * 0xFFFFFFFF + 3 and (ld, le, hl) == (2, 33, 0)
        refused(d.ark355_gr1cs_quotient(ctx, s.g.handle, 0, ptr(zb), m, 0, ptr(out)), B.E_POLY_DEGREE_TOO_LARGE, "degree")
    arity, terms, n, want = shapes(C)["arity4-deg3-N16"]
    with Loaded(lib, ctx, C, 2, m - 2, random_spec(C, rnd, "q", arity, terms, n, m)) as s:
        h = s.g.handle
        good = s.check_def(z, want_dims=want)
        # 2^log_n < n
        assert raw_dims(h, 0, 3)[0] == B.EINVAL
        refused(d.ark355_gr1cs_quotient(ctx, h, 0, ptr(zb), m, 3, ptr(out)), B.EINVAL, "log_n")
        # log_domain + log_ext past the two-adicity: refused before any allocation (2^two_adicity elements would be 2^33 bytes
        # per vector and more)
        rc, deg, ld, le, hl = raw_dims(h, 0, two_adicity)
        assert (rc, deg, ld, le, hl) == (B.E_POLY_DEGREE_TOO_LARGE, 3, two_adicity, 1, 0)
        for fn in (d.ark355_gr1cs_quotient, d.ark355_gr1cs_quotient_dev):
            refused(fn(ctx, h, 0, ptr(zb), m, two_adicity, ptr(out)), B.E_POLY_DEGREE_TOO_LARGE, "radix-2")
            refused(fn(ctx, h, 0, ptr(zb), m, two_adicity + 40, ptr(out)), B.E_POLY_DEGREE_TOO_LARGE)
            refused(fn(ctx, h, 0, ptr(zb), m - 1, 0, ptr(out)), B.E_ASSIGNMENT_MISSING, "shorter")
            refused(fn(ctx, h, 1, ptr(zb), m, 0, ptr(out)), B.EINVAL, "predicate")
            refused(fn(ctx, None, 0, ptr(zb), m, 0, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, None, m, 0, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, ptr(zb), m, 0, None), B.EINVAL, "NULL")
            refused(fn(None, h, 0, ptr(zb), m, 0, ptr(out)), B.EINVAL, message=False)
        assert raw_dims(None, 0, 0)[0] == B.EINVAL and raw_dims(h, 1, 0)[0] == B.EINVAL
        assert d.ark355_gr1cs_quotient_dims(h, 0, 0, None, None, None, None) == 0            # any out pointer may be NULL
        assert raw_dims(h, 0, 0) == (0,) + want + (32,)
        # the context and the handle stay usable
        assert s.g.quotient("q", z) == good
    # n = 0: N = 2, every m_k = 0, h is P(0) / Z on the coset, interpolated
    for terms in ([(5, []), (1, [(0, 3)])], gc.sr1cs_terms(p)):
        spec = {"none": (2, terms, [[], []])}
        with Loaded(lib, ctx, C, 2, m - 2, spec) as s:
            hz = s.check_def(z, want_dims=(degree_of(terms), 1, 1 if degree_of(terms) == 3 else 0))
            assert (hz == bytes(len(hz))) == (terms[0][1] != [])
