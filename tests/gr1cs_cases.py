"""GR1CS cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_gr1cs.py, tests/test_gpu_gr1cs.py): each
drives the C ABI through `snark_amd.GR1CS` / `snark_amd._binding.Lib` and compares with the oracle (oracle/r1cs.py:
PolynomialPredicate, ConstraintSystem, mat_vec_mul, first_unsatisfied_r1cs) on the same seeded inputs.  The library is never
its own expected value; where a case says "agrees with the existing entry" that comparison comes on top of the oracle's.

A system is a `spec`: {label: (arity, terms, matrices)} -- what `to_matrices()[label]` and `get_predicate()` hand out."""
from __future__ import annotations

import json
import os
import random

import numpy as np

from helpers import ROOT, pk_load_from_oracle, r1cs_load_from_rows, z_bytes
from oracle import groth16 as G, r1cs as R, serialize as Z
from snark_amd import GR1CS, _binding as B
from snark_amd.gr1cs import Predicate

CIRCUIT1_X = [1, 2, 3, 0, 1255254]
CIRCUIT1_W = [4, 2, 5, 29, 28, 10, 57, 22022]


def r1cs_terms(p):
    return [(1, [(0, 1), (1, 1)]), (p - 1, [(2, 1)])]          # predicate/mod.rs:115-120


def sr1cs_terms(p):
    return [(1, [(0, 2)]), (p - 1, [(1, 1)])]                  # predicate/mod.rs:123-128


def spec_from_cs(cs):
    mats = cs.to_matrices()
    return {l: (cs.predicates[l].predicate.arity, cs.predicates[l].predicate.terms, mats[l]) for l in mats}


def residual(p, terms, values):
    """PolynomialPredicate::eval in Python integers (next to PolynomialPredicate.is_satisfied, which only says == 0)"""
    acc = 0
    for coeff, mono in terms:
        t = coeff % p
        for vi, e in mono:
            t = t * pow(values[vi], e, p) % p
        acc = (acc + t) % p
    return acc


def fr_list(C, b):
    return [Z.fr_from_mont(C, b[i:i + 32]) for i in range(0, len(b), 32)]


def oracle_walk(C, spec, z):
    """(first unsatisfied (label, row) in sorted-label order or None, {label: per-matrix products}, {label: residuals}) -- the
    `cs`-free walk: mat_vec_mul plus PolynomialPredicate.is_satisfied on every row, labels as in oracle/r1cs.py:345-360"""
    first, prods, res = None, {}, {}
    for label in sorted(spec):
        arity, terms, mats = spec[label]
        pred = R.PolynomialPredicate(C.r, arity, terms)
        mv = [R.mat_vec_mul(M, z, C.r) for M in mats]
        prods[label] = mv
        out = []
        for i in range(len(mats[0]) if mats else 0):
            vals = [mv[k][i] for k in range(arity)]
            r_ = residual(C.r, terms, vals)
            ok = pred.is_satisfied(vals)
            assert (r_ == 0) == ok
            out.append(r_)
            if not ok and first is None:
                first = (label, i)
        res[label] = out
    return first, prods, res


def load(lib, ctx, C, ell, w, spec):
    return GR1CS.from_matrices(C.curve_id, ell, w, spec).load(lib, ctx)


def check_system(lib, ctx, C, ell, w, spec, zs, expect=None):
    """every entry point against the oracle walk, for each assignment of zs; expect: the (label, row) answers known by
    construction, checked against the oracle's as well"""
    g = load(lib, ctx, C, ell, w, spec)
    try:
        assert g.num_constraints() == sum(len(m[0]) if m else 0 for _, _, m in spec.values())
        for k, z in enumerate(zs):
            first, prods, res = oracle_walk(C, spec, z)
            if expect is not None:
                assert first == expect[k], (first, expect[k])
            assert g.which_is_unsatisfied(z) == first, (C.name, k, first)
            assert g.is_satisfied(z) == (first is None)
            for label in spec:
                got = g.mat_vec(label, z)
                assert len(got) == spec[label][0]
                for j, vec in enumerate(got):
                    assert fr_list(C, vec) == prods[label][j], (C.name, label, j)
                assert fr_list(C, g.eval(label, z)) == res[label], (C.name, label)
    finally:
        g.free()


# ---- 1: the reference's Circuit1 (gr1cs/tests/circuit1.rs, tests/mod.rs:17-76) ----------------------------------------------
def circuit1_case(lib, ctx, C):
    cs = R.ConstraintSystem(C.r)
    R.circuit1(cs, CIRCUIT1_X, CIRCUIT1_W)
    cs.finalize()
    spec = spec_from_cs(cs)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "circuit1_matrices.json")))
    as_lists = {l: [[[list(t) for t in row] for row in M] for M in spec[l][2]] for l in spec}
    assert as_lists == golden
    assert spec["R1CS"][0] == 3 and spec["R1CS"][2] == [[], [], []]
    ell, w = cs.num_instance_variables, cs.num_witness_variables
    z = cs.full_assignment()
    assert cs.which_is_unsatisfied() is None
    bad = R.ConstraintSystem(C.r)
    R.circuit1(bad, [4] + CIRCUIT1_X[1:], CIRCUIT1_W)
    bad.finalize()
    label, row = bad.which_is_unsatisfied().split(" - ")
    assert (label, int(row)) == ("poly-predicate-A", 0)
    check_system(lib, ctx, C, ell, w, spec, [z, bad.full_assignment()], expect=[None, (label, int(row))])
    g = load(lib, ctx, C, ell, w, spec)
    try:
        assert [p.label for p in g.predicates if p.n == 0] == ["R1CS"]
        got = g.which_is_unsatisfied(bad.full_assignment())
        assert "%s - %d" % got == bad.which_is_unsatisfied()
    finally:
        g.free()


# ---- systems built forward: satisfied by construction ------------------------------------------------------------------------
class Builder:
    """Every predicate's polynomial ends in `- x_{t-1}` and x_{t-1} appears nowhere else; a row's matrices 0 .. t-2 are random
    linear combinations of the BASE variables (One, the instance, the first witnesses) and its last matrix is k * (a fresh
    witness), so the fresh witness is determined by the row and changing it violates that row and no other."""

    def __init__(self, C, seed, ell=3, base_w=6):
        self.C, self.p, self.rnd = C, C.r, random.Random(seed)
        self.ell, self.base = ell, ell + base_w
        self.inst = [1] + [self.rnd.randrange(self.p) for _ in range(ell - 1)]
        self.wit = [self.rnd.randrange(self.p) for _ in range(base_w)]
        self.spec, self.fresh = {}, {}

    def coeff(self):
        return self.rnd.choice([1, 1, self.p - 1, self.rnd.randrange(1, self.p)])

    def lc(self):
        rnd = self.rnd
        k = rnd.choice([0, 1, 1, 2, 3, 4])                       # 0: the empty row
        row = [(self.coeff(), rnd.randrange(self.base)) for _ in range(k)]
        if k >= 2 and rnd.random() < 0.5:
            row[-1] = (self.coeff(), row[0][1])                  # a repeated column
        if k >= 1 and rnd.random() < 0.3:
            row[0] = (row[0][0], 0)                              # the column of One
        return row

    def z(self):
        return self.inst + self.wit

    def add(self, label, arity, terms, n):
        assert terms[-1] == (self.p - 1, [(arity - 1, 1)])
        assert all(v != arity - 1 for _, mono in terms[:-1] for v, _ in mono)
        mats = [[] for _ in range(arity)]
        rows = []
        for _ in range(n):
            z = self.z()
            vals = []
            for k in range(arity - 1):
                row = self.lc()
                mats[k].append(row)
                vals.append(sum(c * z[j] for c, j in row) % self.p)
            want = residual(self.p, terms[:-1], vals + [0])      # what x_{t-1} has to be
            k = self.coeff()
            rows.append(len(self.inst) + len(self.wit))
            self.wit.append(want * pow(k, -1, self.p) % self.p)
            mats[arity - 1].append([(k, rows[-1])])
        self.spec[label] = (arity, terms, mats)
        self.fresh[label] = rows

    def violated(self, label, row):
        z = self.z()
        z[self.fresh[label][row]] = (z[self.fresh[label][row]] + 1) % self.p
        return z


def random_polynomial(rnd, p, arity, max_deg=7, big_exp=False):
    """terms over x_0 .. x_{t-2} with a constant term, a repeated variable in a monomial and an exponent 0, then - x_{t-1}"""
    terms = [(rnd.randrange(1, p), [])]                          # the constant term
    free = arity - 1
    if free:
        v = rnd.randrange(free)
        terms.append((1, [(v, 2), (v, 1)]))                      # a repeated variable: x_v^3
        terms.append((p - 1, [(rnd.randrange(free), 0), (rnd.randrange(free), max_deg)]))   # exponent 0 contributes 1
        for _ in range(rnd.randrange(1, 4)):
            mono, deg = [], 0
            for _ in range(rnd.randrange(1, 4)):
                e = rnd.randrange(1, 4)
                if deg + e > max_deg:
                    break
                deg += e
                mono.append((rnd.randrange(free), e))
            terms.append((rnd.choice([1, p - 1, rnd.randrange(1, p)]), mono))
        terms.append((1, [(v, 1)] + [(u, 1) for u in range(free)]))          # touches every free variable
        if big_exp:
            terms.append((rnd.randrange(1, p), [(rnd.randrange(free), (1 << 16) + 3)]))
    terms.append((p - 1, [(arity - 1, 1)]))
    return terms


def random_systems_case(lib, ctx, C, rows, seed=0x6121C5):
    """arities 1, 2, 3, 4, 8 and the maximum, degrees up to 7 and one exponent >= 2^16, a predicate with zero rows"""
    b = Builder(C, seed + C.curve_id)
    rnd = b.rnd
    for t in (1, 2, 3, 4, 8, B.GR1CS_MAX_ARITY):
        b.add("arity-%02d" % t, t, random_polynomial(rnd, C.r, t, big_exp=(t == 4)), rows)
    b.add("R1CS", 3, r1cs_terms(C.r), 0)                         # registered by default, no rows
    b.add("empty-of-arity-5", 5, random_polynomial(rnd, C.r, 5), 0)
    labels = [l for l in sorted(b.spec) if b.fresh[l]]
    mid = (labels[2], rows // 2)
    last = (labels[-1], rows - 1)
    zs = [b.z(), b.violated(*mid), b.violated(*last)]
    check_system(lib, ctx, C, b.ell, len(b.wit), b.spec, zs, expect=[None, mid, last])


# ---- 2: label order beats registration order and row index -------------------------------------------------------------------
def label_order_case(lib, ctx, C, rows=8):
    b = Builder(C, 0x1ABE1)
    labels = ["a0", "é", "a", "R1CS", "B"]                   # registration order; sorted: B, R1CS, a, a0, e-acute
    assert sorted(labels) == ["B", "R1CS", "a", "a0", "é"]
    assert sorted(labels) == [x.decode() for x in sorted(l.encode("utf-8") for l in labels)]
    for l in labels:
        if l == "R1CS":
            b.add(l, 3, r1cs_terms(C.r), rows)
        else:
            b.add(l, 2, sr1cs_terms(C.r), rows)

    def both(x, y):
        z = b.violated(*x)
        z[b.fresh[y[0]][y[1]]] = (z[b.fresh[y[0]][y[1]]] + 1) % C.r
        return z
    pairs = [(("a", rows - 1), ("a0", 0)),            # prefix: "a" < "a0", although it fails at a LATER row
             (("R1CS", rows - 2), ("a", 1)),          # case: "R1CS" < "a"
             (("a0", 5), ("é", 0)),              # non-ASCII sorts after ASCII in UTF-8 byte order
             (("B", 3), ("R1CS", 0))]
    zs = [both(x, y) for x, y in pairs]
    check_system(lib, ctx, C, b.ell, len(b.wit), b.spec, zs, expect=[x for x, _ in pairs])


# ---- 5: the reference's SR1CS predicate x0^2 - x1 ----------------------------------------------------------------------------
def sr1cs_case(lib, ctx, C, rows):
    b = Builder(C, 0x5121C5)
    b.add("SR1CS", 2, sr1cs_terms(C.r), rows)
    b.add("R1CS", 3, r1cs_terms(C.r), 0)
    zs = [b.z(), b.violated("SR1CS", rows // 3)]
    check_system(lib, ctx, C, b.ell, len(b.wit), b.spec, zs, expect=[None, ("SR1CS", rows // 3)])


# ---- 4: R1CS through the general path ----------------------------------------------------------------------------------------
def r1cs_general_case(lib, ctx, C, A, Bm, Cm, z, ell, prove=False):
    m = len(z)
    w = m - ell
    spec = {"R1CS": (3, r1cs_terms(C.r), [A, Bm, Cm])}
    zbad = list(z)
    zbad[ell + w // 2] = (zbad[ell + w // 2] + 1) % C.r
    check_system(lib, ctx, C, ell, w, spec, [z, zbad])
    g = load(lib, ctx, C, ell, w, spec)
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, w)
    r1g = g.r1cs_handle()
    pkh = None
    try:
        for zz in (z, zbad):
            first = R.first_unsatisfied_r1cs(A, Bm, Cm, zz, C.r)
            got = g.which_is_unsatisfied(zz)
            assert (-1 if got is None else got[1]) == first
            assert got is None or got[0] == "R1CS"
            zb = z_bytes(C, zz)
            assert lib.is_satisfied(ctx, r1, zb, m) == first            # agrees with the existing entries, both handles
            assert lib.is_satisfied(ctx, r1g, zb, m) == first
            assert g.mat_vec("R1CS", zz) == lib.mat_vec(ctx, r1, zb, m, len(A), 32)
            assert g.mat_vec("R1CS", zz) == lib.mat_vec(ctx, r1g, zb, m, len(A), 32)
        assert lib.dll.ark355_r1cs_domain_size(r1g) == lib.dll.ark355_r1cs_domain_size(r1)
        if prove:
            sz = lib.sizes(C.curve_id)
            pk = G.setup(C, A, Bm, Cm, ell, m, G.Trapdoor(tau=987654321, alpha=5, beta=7, gamma=11, delta=13))
            pkh = pk_load_from_oracle(lib, ctx, C, pk, ell, w, 1 << pk.domain_log)
            r_, s_ = 0x1234567890abcdef % C.r, 0xfedcba0987654321aabbccdd % C.r
            zb = z_bytes(C, z)
            one = lib.prove(ctx, pkh, r1, zb, m, Z.fr_canon(C, r_), Z.fr_canon(C, s_), sz)
            two = lib.prove(ctx, pkh, r1g, zb, m, Z.fr_canon(C, r_), Z.fr_canon(C, s_), sz)
            assert one == two, "the same proof bytes from either handle"
            got = G.Proof(Z.g1_from_raw(C, two[0]), Z.g2_from_raw(C, two[1]), Z.g1_from_raw(C, two[2]))
            exp = G.prove_closed_form(C, pk, z, ell, r_, s_)
            assert got == exp and Z.proof_bytes(C, got) == Z.proof_bytes(C, exp)
    finally:
        if pkh is not None:
            lib.dll.ark355_pk_free(pkh)
        lib.dll.ark355_r1cs_free(r1g)
        lib.dll.ark355_r1cs_free(r1)
        g.free()


def r1cs_refusal_case(lib, ctx, C):
    """ark355_gr1cs_r1cs must not hand out a handle that drops constraints, nor one without "R1CS\""""
    b = Builder(C, 0x4EF05A1)
    b.add("R1CS", 3, r1cs_terms(C.r), 4)
    b.add("s-box", 2, [(1, [(0, 5)]), (C.r - 1, [(1, 1)])], 1)
    for spec, needle in ((b.spec, "s-box"), ({"s-box": b.spec["s-box"]}, "R1CS"),
                         ({"R1CS": (3, [(1, [(0, 1), (1, 1)]), (C.r - 2, [(2, 1)])], b.spec["R1CS"][2])}, "R1CS")):
        g = load(lib, ctx, C, b.ell, len(b.wit), spec)
        try:
            try:
                lib.dll.ark355_r1cs_free(g.r1cs_handle())
                assert False, "must refuse"
            except B.Ark355Error as e:
                assert e.code == B.EINVAL and needle in str(e), str(e)
            assert g.which_is_unsatisfied(b.z()) == oracle_walk(C, spec, b.z())[0]      # context and handle stay usable
        finally:
            g.free()
    # a zero-row second predicate drops nothing: allowed, however "R1CS" was written (term and factor order, an x^0 factor)
    spec = {"R1CS": (3, [(C.r - 1, [(2, 1)]), (1, [(1, 1), (2, 0), (0, 1)])], b.spec["R1CS"][2]),
            "s-box": (2, b.spec["s-box"][1], [[], []])}
    g = load(lib, ctx, C, b.ell, len(b.wit), spec)
    try:
        h = g.r1cs_handle()
        assert lib.is_satisfied(ctx, h, z_bytes(C, b.z()), len(b.z())) == -1
        lib.dll.ark355_r1cs_free(h)
    finally:
        g.free()


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------
def _desc(C, label="p", arity=2, n=1, terms=None, term_ptr=True, var=None, exp=None, mats=True, cols=(1, 2), rp=None):
    terms = sr1cs_terms(C.r) if terms is None else terms
    tp, v, e = [0], [], []
    for _, f in terms:
        v += [a for a, _ in f]
        e += [x for _, x in f]
        tp.append(len(v))
    one = Z.fr_mont(C, 1)
    if mats is True:
        mats = [(np.array(rp if rp is not None else [0] + [1] * n, dtype=np.uint64), np.array([cols[k % len(cols)]], dtype=np.uint32), one)
                for k in range(arity)]
    return (label, arity, n, b"".join(Z.fr_mont(C, c) for c, _ in terms), np.array(tp, dtype=np.uint32) if term_ptr else None,
            np.array(var if var is not None else v, dtype=np.uint32), np.array(exp if exp is not None else e, dtype=np.uint32), mats)


def refusal_case(lib, ctx, C):
    ell, w = 2, 2
    one = Z.fr_mont(C, 1)

    def refused(preds, needle=None, n_ell=ell):
        try:
            lib.gr1cs_free(lib.gr1cs_load(ctx, C.curve_id, n_ell, w, preds))
            assert False, "must be refused: %r" % (needle,)
        except B.Ark355Error as e:
            assert e.code == B.EINVAL, e
            assert needle is None or needle in str(e), str(e)

    def accepted(preds):
        lib.gr1cs_free(lib.gr1cs_load(ctx, C.curve_id, ell, w, preds))

    accepted([_desc(C)])
    refused([_desc(C, arity=0, mats=[])], "arity 0")
    refused([_desc(C, var=[0, 2])], "variable >= arity")
    refused([_desc(C, cols=(1, ell + w))], "column")
    refused([_desc(C, n=2, rp=[0, 2, 1])], "non-decreasing")
    refused([_desc(C, label="x"), _desc(C, label="y"), _desc(C, label="x")], "duplicate")
    refused([_desc(C, label=None)], "label")
    refused([_desc(C, term_ptr=None)[:3] + (one + one, None) + _desc(C)[5:]], "NULL")        # terms without term_ptr
    d = _desc(C)
    refused([d[:3] + (None,) + d[4:]], "NULL")                                                # terms without coefficients
    refused([d[:7] + (None,)], "NULL")                                                        # rows without matrices
    refused([d[:7] + ([(d[7][0][0], None, one), d[7][1]],)], "NULL")                          # entries without columns
    refused([d[:7] + ([(d[7][0][0], d[7][0][1], None), d[7][1]],)], "NULL")                   # entries without coefficients
    refused([d[:7] + ([(None, d[7][0][1], one), d[7][1]],)], "NULL")                          # a matrix without row_ptr
    refused([_desc(C)], "One", n_ell=0)
    # ---- limits: at the limit accepted, one beyond refused ---------------------------------------------------------------------
    T, F, A, P = B.GR1CS_MAX_TERMS, B.GR1CS_MAX_FACTORS, B.GR1CS_MAX_ARITY, B.GR1CS_MAX_PREDICATES
    accepted([_desc(C, arity=A, terms=[(1, [(A - 1, 1)])])])
    refused([_desc(C, arity=A + 1, terms=[(1, [(A, 1)])])], "ARITY")
    accepted([_desc(C, terms=[(1, [(0, 1)])] * T)])
    refused([_desc(C, terms=[(1, [(0, 1)])] * (T + 1))], "TERMS")
    accepted([_desc(C, terms=[(1, [(0, 1)] * (F // 4))] * 4)])
    refused([_desc(C, terms=[(1, [(0, 1)] * (F // 4))] * 4 + [(1, [(1, 1)])])], "FACTORS")
    accepted([_desc(C, label="p%d" % i, n=0) for i in range(P)])
    refused([_desc(C, label="p%d" % i, n=0) for i in range(P + 1)], "PREDICATES")
    refused([_desc(C, n=B.GR1CS_MAX_ROWS + 1, rp=[0, 1])], "ROWS")                # refused before a single row is read
    # exponents may be any uint32_t; a short assignment is AssignmentMissing; the context stays usable throughout
    p = C.r
    spec = {"big": (2, [(1, [(0, 0xFFFFFFFF)]), (p - 1, [(1, 1)])], [[[(1, 1)]], [[(1, 2)]]])}
    z = [1, 3, pow(3, 0xFFFFFFFF, p), 0]
    check_system(lib, ctx, C, ell, w, spec, [z, [1, 3, 5, 0]], expect=[None, ("big", 0)])
    g = load(lib, ctx, C, ell, w, spec)
    try:
        zb = z_bytes(C, z)
        for call in (lambda: lib.gr1cs_which_is_unsatisfied(ctx, g.handle, zb[:-32], 3),
                     lambda: lib.gr1cs_mat_vec(ctx, g.handle, 0, zb[:-32], 3, 2, 1, 32),
                     lambda: lib.gr1cs_eval(ctx, g.handle, 0, zb[:-32], 3, 1, 32)):
            try:
                call()
                assert False, "short assignment must fail"
            except B.Ark355Error as e:
                assert e.code == B.E_ASSIGNMENT_MISSING
        try:
            lib.gr1cs_eval(ctx, g.handle, 1, zb, 4, 1, 32)
            assert False
        except B.Ark355Error as e:
            assert e.code == B.EINVAL
        assert g.which_is_unsatisfied(z) is None
    finally:
        g.free()


def limit_polynomial_case(lib, ctx, C, rows=3):
    """a polynomial AT the limits (maximum arity, terms and factors at once) evaluates like the oracle's"""
    A, T, F = B.GR1CS_MAX_ARITY, B.GR1CS_MAX_TERMS, B.GR1CS_MAX_FACTORS
    rnd = random.Random(0x11317)
    terms, left = [], F - 1
    for k in range(T - 1):
        nf = min(left - (T - 2 - k), rnd.randrange(1, 9)) if k < T - 2 else left
        nf = max(nf, 0)
        terms.append((rnd.choice([1, C.r - 1, rnd.randrange(1, C.r)]), [(rnd.randrange(A - 1), rnd.randrange(0, 4)) for _ in range(nf)]))
        left -= nf
    terms.append((C.r - 1, [(A - 1, 1)]))
    assert len(terms) == T and sum(len(m) for _, m in terms) == F
    b = Builder(C, 0x11318)
    b.add("limits", A, terms, rows)
    check_system(lib, ctx, C, b.ell, len(b.wit), b.spec, [b.z(), b.violated("limits", rows - 1)], expect=[None, ("limits", rows - 1)])


# ---- 7: at scale -- three predicates, CSR built with numpy, the assignment built forward --------------------------------------
class ScaleSystem:
    """R1CS (x0 x1 - x2), a degree-5 gate x0^5 + x1 x2 - x3 (arity 4) and SR1CS (x0^2 - x1) over `n` rows in all.  Every row
    reads base variables at fixed strides and defines one fresh witness (its last argument), so the assignment is satisfied
    by construction and changing a fresh witness violates that row alone."""
    BASE = 64

    def __init__(self, C, n, seed=0x5CA1E):
        self.C, p = C, C.r
        rnd = random.Random(seed)
        self.ell = 2
        base = [rnd.randrange(p) for _ in range(self.BASE)]
        self.sizes = {"R1CS": n - 2 * (n // 3), "deg5": n // 3, "SR1CS": n // 3}
        self.terms = {"R1CS": r1cs_terms(p), "deg5": [(1, [(0, 5)]), (1, [(1, 1), (2, 1)]), (p - 1, [(3, 1)])],
                      "SR1CS": sr1cs_terms(p)}
        # per label: per matrix a list of (coefficient, stride, offset): entry = coefficient * base[(stride * i + offset) % BASE]
        self.pattern = {"R1CS": [[(1, 1, 0), (1, 3, 1)], [(p - 1, 5, 2)]],
                        "deg5": [[(1, 1, 3), (3, 7, 0), (1, 1, 3)], [(1, 5, 1)], [(7, 3, 2), (1, 0, -1)]],
                        "SR1CS": [[(1, 1, 5), (p - 2, 9, 4)]]}
        z = [1, rnd.randrange(p)] + base
        self.first_fresh = {}
        for label in ("R1CS", "deg5", "SR1CS"):
            self.first_fresh[label] = len(z)
            terms, pat = self.terms[label], self.pattern[label]
            for i in range(self.sizes[label]):
                vals = [sum(c * (z[self.col(s, o, i)]) for c, s, o in m) % p for m in pat]
                z.append(residual(p, terms[:-1], vals + [0]))
        self.z = z
        self.w = len(z) - self.ell

    def col(self, stride, offset, i):
        return 0 if offset < 0 else self.ell + (stride * i + offset) % self.BASE          # offset -1: the column of One

    def gr1cs(self):
        C = self.C
        preds = []
        for label in ("deg5", "SR1CS", "R1CS"):                    # registration order differs from the sorted order
            n, rps, cols, cfs = self.sizes[label], [], [], []
            i = np.arange(n, dtype=np.int64)
            for m in self.pattern[label]:
                k = len(m)
                rps.append(np.arange(n + 1, dtype=np.uint64) * k)
                cols.append(np.stack([np.zeros(n, np.int64) if o < 0 else self.ell + (s * i + o) % self.BASE for _, s, o in m], axis=1)
                            .reshape(-1).astype(np.uint32))
                cfs.append(b"".join(Z.fr_mont(C, c) for c, _, _ in m) * n)
            rps.append(np.arange(n + 1, dtype=np.uint64))          # the last matrix: the row's fresh witness
            cols.append((self.first_fresh[label] + i).astype(np.uint32))
            cfs.append(Z.fr_mont(C, 1) * n)
            preds.append(Predicate(label, len(rps), self.terms[label], n, rps, cols, cfs))
        from snark_amd.params import CURVES
        return GR1CS(CURVES[C.curve_id], self.ell, self.w, preds)

    def spec(self):
        """the same system as row lists, for the full oracle walk at small n"""
        out = {}
        for label, pat in self.pattern.items():
            n = self.sizes[label]
            mats = [[[(c, self.col(s, o, i)) for c, s, o in m] for i in range(n)] for m in pat]
            mats.append([[(1, self.first_fresh[label] + i)] for i in range(n)])
            out[label] = (len(mats), self.terms[label], mats)
        return out

    def row_values(self, label, i, z):
        vals = [sum(c * z[self.col(s, o, i)] for c, s, o in m) % self.C.r for m in self.pattern[label]]
        return vals + [z[self.first_fresh[label] + i]]

    def violate(self, z, label, row):
        z[self.first_fresh[label] + row] = (z[self.first_fresh[label] + row] + 1) % self.C.r


def scale_case(lib, ctx, C, n, sample=4096, full_walk=False):
    s = ScaleSystem(C, n)
    g = s.gr1cs().load(lib, ctx)
    try:
        assert g.num_constraints() == n
        zb = bytearray(z_bytes(C, s.z))
        assert g.which_is_unsatisfied(zb) is None
        # three planted violations; sorted labels: R1CS < SR1CS < deg5
        planted = [("deg5", 5), ("SR1CS", s.sizes["SR1CS"] - 1), ("SR1CS", 17)]
        zbad = list(s.z)
        for label, row in planted:
            s.violate(zbad, label, row)
            k = s.first_fresh[label] + row
            zb[32 * k:32 * k + 32] = Z.fr_mont(C, zbad[k])
        assert g.which_is_unsatisfied(zb) == ("SR1CS", 17)
        rnd = random.Random(0x5A3F1E)
        for label in s.sizes:
            rows = set(rnd.sample(range(s.sizes[label]), min(sample, s.sizes[label]))) | {r for l, r in planted if l == label}
            ev = g.eval(label, zb)
            mv = g.mat_vec(label, zb)
            pred = R.PolynomialPredicate(C.r, len(mv), s.terms[label])
            for i in sorted(rows):
                vals = s.row_values(label, i, zbad)
                assert [Z.fr_from_mont(C, v[32 * i:32 * i + 32]) for v in mv] == vals, (label, i)
                r_ = residual(C.r, s.terms[label], vals)
                assert Z.fr_from_mont(C, ev[32 * i:32 * i + 32]) == r_, (label, i)
                assert (r_ == 0) == pred.is_satisfied(vals) == ((label, i) not in planted)
    finally:
        g.free()
    if full_walk:
        zlast = list(s.z)
        s.violate(zlast, "deg5", s.sizes["deg5"] - 1)
        check_system(lib, ctx, C, s.ell, s.w, s.spec(), [s.z, zbad, zlast],
                     expect=[None, ("SR1CS", 17), ("deg5", s.sizes["deg5"] - 1)])
