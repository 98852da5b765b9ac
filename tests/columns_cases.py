"""Column-polynomial cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_columns.py,
tests/test_gpu_columns.py): ark355_lagrange_fr, ark355_gr1cs_mat_vec_t, ark355_gr1cs_columns_at, their `_dev` variants and
ark355_fixed_base_mul_dev (include/ark355.h "Column polynomials of any predicate at a point") against references built from plain
Python integers, oracle.ntt.Domain.lagrange_at and oracle.fields:

  R-sum    sum of c * y[i] mod r over the CSR the test itself loaded (for handles built on the device: the CSR read back with
           ark355_gr1cs_matrix);
  R-setup  ark355_setup asked for u, v, w only: the generator's own, independent code path over the same matrices;
  R-qap    the QAP identity at a point: with a_k = sum_j z_j cols[k][j], P(a_0, .., a_{t-1}) == h(tau) (tau^N - 1), h from
           ark355_gr1cs_quotient and evaluated by Horner's rule.
Every comparison is byte for byte or an exact identity of integers: the arithmetic is exact.  `io` carries the tier's device
memory, as in tests/sr1cs_cases.py.

Not reachable at a test's size, and so not covered: the refusal of more than 2^32 - 1 non-zeros, ARK355_ENOMEM, and a handle of
another device (both tiers have one device)."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import gr1cs_cases as gc
import lcmap_cases as lcc
import quotient_cases as qc
import sr1cs_cases as sc
from helpers import r1cs_load_from_rows, z_bytes
from oracle import r1cs as R, serialize as Z, synthetic as S
from oracle.ntt import Domain
from snark_amd import GR1CS, LcSystem, _binding as B
from snark_amd.gr1cs import Predicate
from snark_amd.params import CURVES as PRODUCT_CURVES

LANE_MAX, CHUNK = 64, 2048                  # COLS_LANE_MAX's default and COLGATHER_CHUNK (snark_amd/csrc/colgather_impl.cuh)
LINEAR = [(1, [(0, 1)])]                    # a polynomial for systems whose polynomial does not matter: x0


def mont(C, ints):
    return S._mont_bytes(C.r, list(ints))


def tau_bytes(tau):
    return int(tau).to_bytes(32, "little")


def two_adicity(C):
    return ((C.r - 1) & -(C.r - 1)).bit_length() - 1


# ---- R-sum ---------------------------------------------------------------------------------------------------------------------
def r_sum(C, mats, y, m):
    """[[sum over the stored entries (i, j, c) of M_k of c y[i]] for j < m] for every matrix"""
    p = C.r
    out = []
    for M in mats:
        col = [0] * m
        for i, row in enumerate(M):
            for c, j in row:
                col[j] += c * y[i]
        out.append([v % p for v in col])
    return out


def check_mat_vec_t(C, g, label, mats, y, tag):
    want = [mont(C, v) for v in r_sum(C, mats, y, g.m)]
    got = g.mat_vec_t(label, y)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (C.name, tag, "matrix %d" % k, qc.first_difference(a, b))
    return got


def check_columns_at(C, g, label, mats, tau, log_n=0, tag=""):
    """columns_at against R-sum with lagrange_at, and against mat_vec_t(lagrange_fr(..)): the same bytes"""
    n = len(mats[0]) if mats else 0
    log_domain = log_n or max(1, (max(n, 2) - 1).bit_length())
    lag = Domain(C, log_domain).lagrange_at(tau)
    want = [mont(C, v) for v in r_sum(C, mats, lag[:n], g.m)]
    got = g.columns_at(label, tau, log_n)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (C.name, tag, "matrix %d" % k, qc.first_difference(a, b))
    lb = g.lib.lagrange_fr(g.ctx, C.curve_id, log_domain, tau_bytes(tau))
    assert lb == mont(C, lag), (C.name, tag, "lagrange_fr")
    assert g.mat_vec_t(label, lb[:32 * n]) == got, (C.name, tag, "mat_vec_t(lagrange_fr) != columns_at")
    return got


# ---- 1: mat_vec_t against R-sum ------------------------------------------------------------------------------------------------
def arity_case(lib, ctx, C, arity):
    rnd = random.Random("cols/arity/%d/%d" % (arity, C.curve_id))
    n, m = 37, 11
    spec = qc.random_spec(C, rnd, "p", arity, LINEAR, n, m)
    g = gc.load(lib, ctx, C, 3, m - 3, spec)
    try:
        check_mat_vec_t(C, g, "p", spec["p"][2], [rnd.randrange(C.r) for _ in range(n)], "arity %d" % arity)
    finally:
        g.free()


def edges_spec(C, seed=1):
    """a row with a repeated column, a stored zero, an empty row, an empty matrix, a column without entries (5) and the
    coefficient one next to general ones"""
    p = C.r
    rnd = random.Random(0xED6E + seed)
    c = lambda: rnd.randrange(2, p)                            # noqa: E731
    M0 = [[(c(), 1), (c(), 1), (1, 0)], [(0, 2)], [], [(1, 3), (p - 1, 3), (c(), 4)]]
    M1 = [[], [], [], []]
    M2 = [[(1, 0)], [(1, 0), (c(), 4)], [(c(), 2)], []]
    return {"e": (3, gc.r1cs_terms(p), [M0, M1, M2])}, rnd


def edges_case(lib, ctx, C):
    p = C.r
    spec, rnd = edges_spec(C)
    g = gc.load(lib, ctx, C, 2, 4, spec)
    try:
        got = check_mat_vec_t(C, g, "e", spec["e"][2], [rnd.randrange(p) for _ in range(4)], "edges")
        assert got[1] == bytes(32 * 6) and got[0][5 * 32:] == bytes(32) and got[0][2 * 32:3 * 32] == bytes(32)
    finally:
        g.free()
    # n = 0: all zero, whatever y is
    g = gc.load(lib, ctx, C, 2, 4, {"none": (2, LINEAR, [[], []])})
    try:
        assert g.mat_vec_t("none", b"") == [bytes(32 * 6)] * 2
        assert g.columns_at("none", 12345) == [bytes(32 * 6)] * 2
    finally:
        g.free()
    # m = 1: the constant column alone
    rows = [[(rnd.randrange(p), 0)] * (i % 3) for i in range(9)]
    g = gc.load(lib, ctx, C, 1, 0, {"one": (1, LINEAR, [rows])})
    try:
        check_mat_vec_t(C, g, "one", [rows], [rnd.randrange(p) for _ in range(9)], "m = 1")
    finally:
        g.free()


def several_predicates_case(lib, ctx, C):
    """three predicates whose labels are not in sorted order: each is addressed by the caller's index"""
    rnd = random.Random(0x5E7 + C.curve_id)
    m = 9
    spec = {}
    for label, arity, n in (("zeta", 2, 5), ("alpha", 4, 12), ("mid", 1, 3)):
        spec.update(qc.random_spec(C, rnd, label, arity, LINEAR, n, m))
    g = gc.load(lib, ctx, C, 2, m - 2, spec)
    try:
        for label in ("mid", "zeta", "alpha"):
            n = len(spec[label][2][0])
            check_mat_vec_t(C, g, label, spec[label][2], [rnd.randrange(C.r) for _ in range(n)], label)
            check_columns_at(C, g, label, spec[label][2], rnd.randrange(C.r), tag=label)
    finally:
        g.free()


# ---- 2: column lengths on both sides of both thresholds --------------------------------------------------------------------------
LENGTHS = (1, 2, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
ROWS = 5000                                 # the constant column of matrix 0: three chunks


def lengths_spec(C, seed=0):
    """matrix 0: column 0 in every one of the 5000 rows, column 1 + q in the first LENGTHS[q] rows; matrix 1: columns of 1, 2, 3
    and 2 CHUNK + 1 entries (the lengths around COLS_LANE_MAX = 2), the long one at the END of the rows"""
    p = C.r
    rnd = random.Random(0x1E96 + seed)
    palette = [1, p - 1] + [rnd.randrange(p) for _ in range(14)]
    M0 = [[(rnd.choice(palette), 0)] + [(rnd.choice(palette), 1 + q) for q, L in enumerate(LENGTHS) if i < L] for i in range(ROWS)]
    M1 = [[(rnd.choice(palette), q) for q, L in enumerate((1, 2, 3)) if i < L] +
          ([(rnd.choice(palette), 7)] if i >= ROWS - (2 * CHUNK + 1) else []) for i in range(ROWS)]
    y = [rnd.randrange(p) for _ in range(ROWS)]
    return {"len": (2, LINEAR, [M0, M1])}, y


def lengths_case(lib, ctx, C, policy):
    spec, y = lengths_spec(C)
    m = 1 + len(LENGTHS) + 2
    g = gc.load(lib, ctx, C, 1, m - 1, spec)
    try:
        assert lib.ctx_get_policy(ctx, "COLS_LANE_MAX") == LANE_MAX
        default = check_mat_vec_t(C, g, "len", spec["len"][2], y, "default")
        policy.setenv("ARK355_COLS_LANE_MAX", 2)
        assert g.mat_vec_t("len", y) == default, (C.name, "COLS_LANE_MAX = 2 changed the bytes")
        policy.setenv("ARK355_COLS_LANE_MAX", 0)               # <= 0: the default
        assert g.mat_vec_t("len", y) == default
    finally:
        g.free()


# ---- 3: lagrange_fr ----------------------------------------------------------------------------------------------------------------
def lagrange_case(lib, ctx, C, log_n):
    p = C.r
    dom = Domain(C, log_n)
    rnd = random.Random(0x1A6 + log_n + C.curve_id)
    N, rinv, one = 1 << log_n, pow(1 << 256, -1, p), Z.fr_mont(C, 1)
    for tau in (0, 1, pow(dom.omega, 5, p), p - 1, rnd.randrange(p)):
        want = mont(C, dom.lagrange_at(tau))
        got = lib.lagrange_fr(ctx, C.curve_id, log_n, tau_bytes(tau))
        assert got == want, (C.name, log_n, tau, qc.first_difference(got, want))
        assert sum(qc.raw_list(got)) * rinv % p == 1           # oracle-free: the L_i sum to the constant polynomial 1
    # tau = w^5 inside the domain: the indicator vector of position 5 mod N, whatever the oracle says
    got = lib.lagrange_fr(ctx, C.curve_id, log_n, tau_bytes(pow(dom.omega, 5, p)))
    assert got == b"".join(one if i == 5 % N else bytes(32) for i in range(N))


# ---- 4: columns_at against R-sum -----------------------------------------------------------------------------------------------
def columns_at_case(lib, ctx, C):
    p = C.r
    rnd = random.Random(0xC01A + C.curve_id)
    n, m = 70, 9
    spec = qc.random_spec(C, rnd, "q", 2, gc.sr1cs_terms(p), n, m)
    mats = spec["q"][2]
    g = gc.load(lib, ctx, C, 2, m - 2, spec)
    try:
        tau = rnd.randrange(p)
        c0 = check_columns_at(C, g, "q", mats, tau, tag="70 rows in 128")
        assert check_columns_at(C, g, "q", mats, tau, log_n=7, tag="explicit 7") == c0
        assert check_columns_at(C, g, "q", mats, tau, log_n=9, tag="explicit 9") != c0
        # tau inside the domain selects row 5 of each matrix
        w5 = pow(Domain(C, 7).omega, 5, p)
        got = check_columns_at(C, g, "q", mats, w5, tag="tau in H")
        rows = [mont(C, r_sum(C, [[M[5]]], [1], m)[0]) for M in mats]
        assert got == rows
    finally:
        g.free()


# ---- 5: columns_at against R-setup -----------------------------------------------------------------------------------------------
def _setup_uvw(lib, ctx, C, r1, ell, w, tau):
    N = lib.dll.ark355_r1cs_domain_size(r1)
    td = b"".join(Z.fr_canon(C, x) for x in (tau, 5, 7, 11, 13))
    got, _ = lib.setup(ctx, r1, Z.g1_raw(C, C.g1_gen), Z.g2_raw(C, C.g2_gen), td, (ell, w, N), lib.sizes(C.curve_id),
                       want=("u", "v", "w"), want_pk=False)
    return [got[k].tobytes() for k in ("u", "v", "w")]


def assert_mont_equals_canonical(C, got_mont, want_canon, tag):
    """element for element: the Montgomery image times R^-1 is the canonical value"""
    p, rinv = C.r, pow(1 << 256, -1, C.r)
    assert len(got_mont) == len(want_canon), tag
    for i in range(0, len(got_mont), 32):
        a = int.from_bytes(got_mont[i:i + 32], "little") * rinv % p
        assert a == int.from_bytes(want_canon[i:i + 32], "little"), (tag, "element %d" % (i // 32))


def setup_case(lib, ctx, C, n, tau=987654321):
    """A with the ell instance rows e_j appended, B and C with empty rows: columns_at == setup's u, v, w"""
    p = C.r
    A, Bm, Cm, z, ell = S.mulchain_direct(p, n)
    m = len(z)
    A2 = A + [[(1, j)] for j in range(ell)]
    B2, C2 = Bm + [[] for _ in range(ell)], Cm + [[] for _ in range(ell)]
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, m - ell)
    g = gc.load(lib, ctx, C, ell, m - ell, {"R1CS": (3, gc.r1cs_terms(p), [A2, B2, C2])})
    try:
        uvw = _setup_uvw(lib, ctx, C, r1, ell, m - ell, tau)
        cols = g.columns_at("R1CS", tau)
        for k in range(3):
            assert_mont_equals_canonical(C, cols[k], uvw[k], (C.name, n, "uvw"[k]))
    finally:
        g.free()
        lib.dll.ark355_r1cs_free(r1)


def extended_r1cs(C, ell, w, mats):
    """the CSR arrays of an R1CS with the instance rows appended to A, as a loaded-to-be GR1CS (numpy, for sizes where row
    lists are slow)"""
    n = len(mats[0][0]) - 1
    one = Z.fr_mont(C, 1)
    rp0, col0, cf0 = mats[0]
    ext = [(np.concatenate([rp0, rp0[-1] + np.arange(1, ell + 1, dtype=np.uint64)]),
            np.concatenate([col0, np.arange(ell, dtype=np.uint32)]), bytes(cf0) + one * ell)]
    for rp, col, cf in mats[1:]:
        ext.append((np.concatenate([rp, np.full(ell, rp[-1], dtype=np.uint64)]), col, cf))
    pred = Predicate("R1CS", 3, gc.r1cs_terms(C.r), n + ell, [e[0] for e in ext], [e[1] for e in ext], [e[2] for e in ext])
    return GR1CS(PRODUCT_CURVES[C.curve_id], ell, w, [pred])


def setup_csr_case(lib, ctx, C, ell, w, mats, tau=987654321):
    n = len(mats[0][0]) - 1
    r1 = lib.r1cs_load(ctx, C.curve_id, n, ell, w, mats)
    g = extended_r1cs(C, ell, w, mats).load(lib, ctx)
    try:
        uvw = _setup_uvw(lib, ctx, C, r1, ell, w, tau)
        cols = g.columns_at("R1CS", tau)
        for k in range(3):
            assert_mont_equals_canonical(C, cols[k], uvw[k], (C.name, n, "uvw"[k]))
    finally:
        g.free()
        lib.dll.ark355_r1cs_free(r1)


# ---- 6: R-qap --------------------------------------------------------------------------------------------------------------------
def r_qap(C, terms, cols, z, h, log_domain, tau, tag):
    """P(a_0, ..) == h(tau) (tau^N - 1) with a_k = sum_j z_j cols[k][j]; cols and h as lists of integers"""
    p = C.r
    a = [sum(zj * cj for zj, cj in zip(z, col)) % p for col in cols]
    h_tau = 0
    for c in reversed(h):
        h_tau = (h_tau * tau + c) % p
    assert gc.residual(p, terms, a) == h_tau * (pow(tau, 1 << log_domain, p) - 1) % p, (C.name, tag, "P(a) != h(tau) Z(tau)")


def qap_tau(C, rnd, log_len, satisfied):
    """X^N - 1 divides P(m_0, ..) only for an assignment that satisfies all N rows: then tau is random in the whole field.
    Otherwise h is defined by the coset g H_{DN} alone, and tau is a random point of it (quotient_cases.r_pt)."""
    if satisfied:
        return rnd.randrange(2, C.r)
    big = Domain(C, log_len)
    return big.g * pow(big.omega, rnd.randrange(big.n), C.r) % C.r


def arity4_deg3(C):
    """x0 x1 x2 + c x0 - x3 over 6 rows: no constant term, so the two padded rows of N = 8 hold as well"""
    p = C.r
    b = gc.Builder(C, 0xA4D3 + C.curve_id)
    b.add("deg3a4", 4, [(1, [(0, 1), (1, 1), (2, 1)]), (b.coeff(), [(0, 1)]), (p - 1, [(3, 1)])], 6)
    return b.ell, len(b.wit), b.spec, b.z()


def qap_systems(C):
    out = {k: v[:4] for k, v in qc.satisfied_systems(C).items() if k != "random-deg3-N8"}
    out["random-deg3-arity4-N8"] = arity4_deg3(C)
    return out


def qap_case(lib, ctx, C, name):
    ell, w, spec, z = qap_systems(C)[name]
    rnd = random.Random("qap/%s/%d" % (name, C.curve_id))
    g = gc.load(lib, ctx, C, ell, w, spec)
    try:
        label = next(iter(spec))
        assert g.which_is_unsatisfied(z) is None
        d, log_domain, log_ext, h_len = g.quotient_dims(label)
        if name.startswith("random"):
            assert (spec[label][0], d, log_domain) == (4, 3, 3)
        h = qc.fr_list(C, g.quotient(label, z))
        for _ in range(2):
            tau = qap_tau(C, rnd, log_domain + log_ext, True)
            cols = [qc.fr_list(C, c) for c in check_columns_at(C, g, label, spec[label][2], tau, tag=name)]
            r_qap(C, spec[label][1], cols, z, h, log_domain, tau, name)
    finally:
        g.free()


def sr1cs_chain_on(lib, ctx, C, io, s, zb, m, seed, satisfied):
    """ark355_sr1cs_assignment_dev -> ark355_gr1cs_quotient_dev and ark355_gr1cs_columns_at_dev on the borrowed system, device
    pointers throughout; the columns also against R-sum over the matrices read back"""
    n_ell, n_w, rows, _ = s.dims
    mp = n_ell + n_w
    terms = gc.sr1cs_terms(C.r)
    d, log_domain, log_ext, h_len = s.system.quotient_dims(sc.SR1CS_LABEL)
    rnd = random.Random(seed)
    tau = qap_tau(C, rnd, log_domain + log_ext, satisfied)
    d_z, k1 = io.to_dev(zb)
    d_zp, k2 = io.alloc(mp * 32)
    d_h, k3 = io.alloc(h_len * 32)
    d_c, k4 = io.alloc(2 * mp * 32)
    s.assignment_dev(d_z, m, d_zp)
    s.system.quotient_dev(sc.SR1CS_LABEL, d_zp, mp, d_h)
    s.system.columns_at_dev(sc.SR1CS_LABEL, tau, d_c)
    zp, h, cb = io.read(k2, mp * 32), io.read(k3, h_len * 32), io.read(k4, 2 * mp * 32)
    assert (s.system.which_is_unsatisfied(zp) is None) == satisfied
    scale = pow(1 << 256, -1, C.r)                             # raw Montgomery integers: one factor R^-1 per linear sum
    cols = [[v * scale % C.r for v in qc.raw_list(cb[k * mp * 32:(k + 1) * mp * 32])] for k in range(2)]
    r_qap(C, terms, cols, [v * scale % C.r for v in qc.raw_list(zp)], [v * scale % C.r for v in qc.raw_list(h)], log_domain, tau,
          "sr1cs chain")
    assert b"".join(s.system.columns_at(sc.SR1CS_LABEL, tau)) == cb            # the host entry: the same bytes
    if rows <= 6000:                                                           # R-sum over the CSR the device built
        mats = [sc.rows_from_csr(C, *mk) for mk in s.matrices()]
        lag = Domain(C, log_domain).lagrange_at(tau)
        assert cb == b"".join(mont(C, v) for v in r_sum(C, mats, lag[:rows], mp)), (C.name, "columns of the SR1CS system")


def sr1cs_chain_case(lib, ctx, C, io, A, Bm, Cm, z, ell, seed=0xC7A0):
    m = len(z)
    s, _ = sc.build(lib, ctx, C, A, Bm, Cm, ell, m)
    try:
        sr1cs_chain_on(lib, ctx, C, io, s, z_bytes(C, z), m, seed, R.first_unsatisfied_r1cs(A, Bm, Cm, z, C.r) == -1)
    finally:
        s.free()


def from_lcs_case(lib, ctx, C, rows=20):
    """a handle from ark355_gr1cs_from_lcs against the same system through ark355_gr1cs_load: the same bytes, and R-qap"""
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
        copy = GR1CS(PRODUCT_CURVES[C.curve_id], g.ell, g.w,
                     [Predicate(label, pred.arity, pred.terms, pred.n, [a for a, _, _ in mats], [b for _, b, _ in mats],
                                [c for _, _, c in mats])]).load(lib, ctx)
        try:
            rnd = random.Random(0x1C5 + C.curve_id)
            d, log_domain, log_ext, h_len = g.quotient_dims(label)
            tau = qap_tau(C, rnd, log_domain + log_ext, satisfied)
            rows_k = [sc.rows_from_csr(C, *mk) for mk in mats]
            got = check_columns_at(C, g, label, rows_k, tau, tag="from_lcs")
            assert copy.columns_at(label, tau) == got
            y = [rnd.randrange(C.r) for _ in range(pred.n)]
            assert check_mat_vec_t(C, g, label, rows_k, y, "from_lcs") == copy.mat_vec_t(label, y)
            r_qap(C, gc.r1cs_terms(C.r), [qc.fr_list(C, c) for c in got], z, qc.fr_list(C, g.quotient(label, z)), log_domain, tau,
                  "from_lcs")
        finally:
            copy.free()
    finally:
        g.free()


# ---- 7: `_dev` variants ----------------------------------------------------------------------------------------------------------
def dev_case(lib, ctx, C, io):
    """the same bytes as the host variants, into buffers the tier filled with 0xA5"""
    p = C.r
    rnd = random.Random(0xDE7 + C.curve_id)
    n, m = 70, 9
    spec = qc.random_spec(C, rnd, "q", 3, gc.r1cs_terms(p), n, m)
    g = gc.load(lib, ctx, C, 2, m - 2, spec)
    try:
        y = mont(C, [rnd.randrange(p) for _ in range(n)])
        tau = rnd.randrange(p)
        d_y, k0 = io.to_dev(y)
        d_o, k1 = io.alloc(3 * m * 32 + 64)
        g.mat_vec_t_dev("q", d_y, n, d_o)
        got = io.read(k1, 3 * m * 32 + 64)
        assert got[:3 * m * 32] == b"".join(g.mat_vec_t("q", y)) and got[3 * m * 32:] == b"\xA5" * 64
        d_o, k2 = io.alloc(3 * m * 32 + 64)
        g.columns_at_dev("q", tau, d_o)
        got = io.read(k2, 3 * m * 32 + 64)
        assert got[:3 * m * 32] == b"".join(g.columns_at("q", tau)) and got[3 * m * 32:] == b"\xA5" * 64
        for t in (tau, pow(Domain(C, 7).omega, 5, p)):
            d_o, k3 = io.alloc(128 * 32 + 64)
            lib.lagrange_fr_dev(ctx, C.curve_id, 7, tau_bytes(t), d_o)
            got = io.read(k3, 128 * 32 + 64)
            assert got[:128 * 32] == lib.lagrange_fr(ctx, C.curve_id, 7, tau_bytes(t)) and got[128 * 32:] == b"\xA5" * 64
    finally:
        g.free()


# ---- 8: ark355_fixed_base_mul_dev ----------------------------------------------------------------------------------------------
FB_TABLE_MIN = 512                          # from this many scalars on the entry builds its window table (api_impl.cuh)


def fixed_base_case(lib, ctx, C, io, group, n):
    p = C.r
    rnd = random.Random(0xFB + 7 * group + n + C.curve_id)
    ks = ([0, 1, p - 1] + [rnd.randrange(p) for _ in range(n)])[:n]
    base = Z.g1_raw(C, C.g1_gen) if group == 1 else Z.g2_raw(C, C.g2_gen)
    size = lib.sizes(C.curve_id)["g1" if group == 1 else "g2"]
    canon = b"".join(Z.fr_canon(C, k) for k in ks)
    want = lib.fixed_base_mul(ctx, C.curve_id, group, base, canon, n, size)
    assert want[:size] == bytes(size)                           # 0 * base: the all-zero point
    assert want[size:2 * size] == base
    for scalars, is_mont in ((canon, 0), (mont(C, ks), 1)):
        d_k, keep = io.to_dev(scalars)
        got = lib.fixed_base_mul_dev(ctx, C.curve_id, group, base, d_k, n, is_mont, size)
        assert got == want, (C.name, group, n, "mont" if is_mont else "canonical")


def key_points_case(lib, ctx, C, io, n=1030, tau=987654321):
    """matrices -> key scalars -> key points without the host: columns_at_dev -> fixed_base_mul_dev(scalars_mont = 1) equals
    ark355_setup's a_query"""
    p = C.r
    A, Bm, Cm, z, ell = S.mulchain_direct(p, n)
    m = len(z)
    A2 = A + [[(1, j)] for j in range(ell)]
    B2, C2 = Bm + [[] for _ in range(ell)], Cm + [[] for _ in range(ell)]
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, m - ell)
    g = gc.load(lib, ctx, C, ell, m - ell, {"R1CS": (3, gc.r1cs_terms(p), [A2, B2, C2])})
    try:
        sizes = lib.sizes(C.curve_id)
        base = Z.g1_raw(C, C.g1_gen)
        td = b"".join(Z.fr_canon(C, x) for x in (tau, 5, 7, 11, 13))
        want, _ = lib.setup(ctx, r1, base, Z.g2_raw(C, C.g2_gen), td, (ell, m - ell, lib.dll.ark355_r1cs_domain_size(r1)), sizes,
                            want=("a_query",), want_pk=False)
        d_c, keep = io.alloc(3 * m * 32)
        g.columns_at_dev("R1CS", tau, d_c)
        got = lib.fixed_base_mul_dev(ctx, C.curve_id, 1, base, d_c, m, 1, sizes["g1"])
        assert got == want["a_query"].tobytes(), (C.name, "a_query")
    finally:
        g.free()
        lib.dll.ark355_r1cs_free(r1)


# ---- 9: dirty scratch ----------------------------------------------------------------------------------------------------------
def dirty_sequence(lib, ctx, C):
    """in a fresh context: a large call, a small one, a small one with other data, the large one again, then a refusal followed
    by a good call; every step against R-sum"""
    p = C.r
    big, y_big = lengths_spec(C, seed=C.curve_id)
    m_big = 1 + len(LENGTHS) + 2
    gb = gc.load(lib, ctx, C, 1, m_big - 1, big)
    s1, r1 = edges_spec(C, seed=2)
    s2, r2 = edges_spec(C, seed=3)
    g1 = gc.load(lib, ctx, C, 2, 4, s1)
    g2 = gc.load(lib, ctx, C, 2, 4, s2)
    try:
        first = check_mat_vec_t(C, gb, "len", big["len"][2], y_big, "large")
        check_mat_vec_t(C, g1, "e", s1["e"][2], [r1.randrange(p) for _ in range(4)], "small")
        check_columns_at(C, g1, "e", s1["e"][2], r1.randrange(p), tag="small at tau")
        check_mat_vec_t(C, g2, "e", s2["e"][2], [r2.randrange(p) for _ in range(4)], "small, other data")
        check_columns_at(C, g2, "e", s2["e"][2], pow(Domain(C, 2).omega, 3, p), tag="small, tau in H")
        assert check_mat_vec_t(C, gb, "len", big["len"][2], y_big, "large again") == first
        try:
            g1.columns_at("e", p)                              # tau = r
            raise AssertionError("tau = r was accepted")
        except B.Ark355Error as e:
            assert e.code == B.EINVAL and "tau" in str(e)
        check_columns_at(C, g2, "e", s2["e"][2], r2.randrange(p), tag="after the refusal")
    finally:
        for g in (gb, g1, g2):
            g.free()


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------
def refusals_case(lib, ctx, C):
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    rnd = random.Random(0x2EF + C.curve_id)
    n, m = 13, 9
    spec = qc.random_spec(C, rnd, "q", 2, gc.sr1cs_terms(p), n, m)
    y = [rnd.randrange(p) for _ in range(n)]
    yb = np.frombuffer(mont(C, y), dtype=np.uint8).copy()
    out = np.zeros(32 * 1024, dtype=np.uint8)
    tau = np.frombuffer(tau_bytes(rnd.randrange(p)), dtype=np.uint8).copy()
    tau_r = np.frombuffer(tau_bytes(p), dtype=np.uint8).copy()
    tau_max = np.full(32, 0xFF, dtype=np.uint8)
    adic = two_adicity(C)

    def refused(rc, code, needle=None, message=True):
        assert rc == code, (rc, code)
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg

    g = gc.load(lib, ctx, C, 2, m - 2, spec)
    try:
        h = g.handle
        good = check_mat_vec_t(C, g, "q", spec["q"][2], y, "before")
        for fn in (d.ark355_gr1cs_mat_vec_t, d.ark355_gr1cs_mat_vec_t_dev):
            refused(fn(ctx, None, 0, ptr(yb), n, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, None, n, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, ptr(yb), n, None), B.EINVAL, "NULL")
            refused(fn(ctx, h, 1, ptr(yb), n, ptr(out)), B.EINVAL, "predicate")
            refused(fn(ctx, h, 0, ptr(yb), n - 1, ptr(out)), B.EINVAL, "shorter")
            refused(fn(None, h, 0, ptr(yb), n, ptr(out)), B.EINVAL, message=False)
        for fn in (d.ark355_gr1cs_columns_at, d.ark355_gr1cs_columns_at_dev):
            refused(fn(ctx, None, 0, ptr(tau), 0, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, None, 0, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, h, 0, ptr(tau), 0, None), B.EINVAL, "NULL")
            refused(fn(ctx, h, 1, ptr(tau), 0, ptr(out)), B.EINVAL, "predicate")
            refused(fn(ctx, h, 0, ptr(tau_r), 0, ptr(out)), B.EINVAL, "tau")
            refused(fn(ctx, h, 0, ptr(tau_max), 0, ptr(out)), B.EINVAL, "tau")
            refused(fn(ctx, h, 0, ptr(tau), 3, ptr(out)), B.EINVAL, "log_n")
            refused(fn(ctx, h, 0, ptr(tau), adic + 1, ptr(out)), B.E_POLY_DEGREE_TOO_LARGE, "radix-2")
            refused(fn(None, h, 0, ptr(tau), 0, ptr(out)), B.EINVAL, message=False)
        for fn in (d.ark355_lagrange_fr, d.ark355_lagrange_fr_dev):
            refused(fn(ctx, C.curve_id, 3, None, ptr(out)), B.EINVAL, "NULL")
            refused(fn(ctx, C.curve_id, 3, ptr(tau), None), B.EINVAL, "NULL")
            refused(fn(ctx, C.curve_id, 3, ptr(tau_r), ptr(out)), B.EINVAL, "tau")
            refused(fn(ctx, 77, 3, ptr(tau), ptr(out)), B.EINVAL, "curve")
            refused(fn(ctx, C.curve_id, adic + 1, ptr(tau), ptr(out)), B.E_POLY_DEGREE_TOO_LARGE, "radix-2")
        sz = lib.sizes(C.curve_id)["g1"]
        base = np.frombuffer(Z.g1_raw(C, C.g1_gen), dtype=np.uint8).copy()
        refused(d.ark355_fixed_base_mul_dev(ctx, C.curve_id, 1, None, ptr(yb), 2, 1, ptr(out)), B.EINVAL, "NULL")
        refused(d.ark355_fixed_base_mul_dev(ctx, C.curve_id, 1, ptr(base), None, 2, 1, ptr(out)), B.EINVAL, "NULL")
        refused(d.ark355_fixed_base_mul_dev(ctx, C.curve_id, 1, ptr(base), ptr(yb), 2, 1, None), B.EINVAL, "NULL")
        refused(d.ark355_fixed_base_mul_dev(ctx, C.curve_id, 3, ptr(base), ptr(yb), 2, 1, ptr(out)), B.EINVAL, "group")
        assert sz <= len(out)
        # the context and the handle stay usable
        assert g.mat_vec_t("q", y) == good
        check_columns_at(C, g, "q", spec["q"][2], rnd.randrange(p), tag="after the refusals")
    finally:
        g.free()
    # t m + 1 >= 2^32: sixteen empty matrices over 2^28 columns; refused before anything of that size is allocated
    wide = gc.load(lib, ctx, C, 1, (1 << 28) - 1, {"wide": (16, LINEAR, [[] for _ in range(16)])})
    try:
        refused(d.ark355_gr1cs_mat_vec_t(ctx, wide.handle, 0, ptr(yb), 0, ptr(out)), B.EINVAL, "2^32")
        refused(d.ark355_gr1cs_columns_at_dev(ctx, wide.handle, 0, ptr(tau), 0, ptr(out)), B.EINVAL, "2^32")
    finally:
        wide.free()
