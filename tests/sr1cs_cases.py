"""Square R1CS cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_sr1cs.py, tests/test_gpu_sr1cs.py): the
device adapter (include/ark355.h "Square R1CS", snark_amd.SR1CS) against a transliteration of the reference's
`Sr1csAdapter::r1cs_to_sr1cs_with_assignment` (relations/src/sr1cs/mod.rs:85-116, :191-265) onto oracle/r1cs.py's
ConstraintSystem.  The transliteration keeps the adapter's two maps and its allocation order and knows nothing of the closed
form the kernels use; the library is never its own expected value.

`io` carries the tier's device memory: io.to_dev(bytes) -> (pointer, keepalive), io.alloc(nbytes) -> (pointer, keepalive),
io.read(keepalive, nbytes) -> bytes."""
from __future__ import annotations

import ctypes
import random

import numpy as np

from helpers import csr_from_rows, r1cs_load_from_rows, z_bytes
from oracle import r1cs as R, serialize as Z, synthetic as S
from snark_amd import SR1CS, _binding as B

SR1CS_LABEL = "SR1CS"


class HostIO:
    """the emulator's "device" memory is host memory"""

    @staticmethod
    def to_dev(b):
        a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
        return a.ctypes.data, a

    @staticmethod
    def alloc(nbytes):
        a = np.full(max(1, nbytes), 0xA5, dtype=np.uint8)
        return a.ctypes.data, a

    @staticmethod
    def read(keep, nbytes):
        return keep.tobytes()[:nbytes]


# ---- the reference side ------------------------------------------------------------------------------------------------------
def sr1cs_terms(p):
    return [(1, [(0, 2)]), (p - 1, [(1, 1)])]                  # predicate/mod.rs:123-128 (new_sr1cs_predicate)


class Adapted:
    """what r1cs_to_sr1cs_with_assignment leaves behind, plus its two maps"""

    def __init__(self, cs, public_variables, witness_variables, old_m):
        self.cs = cs
        self.ell, self.w = cs.num_instance_variables, cs.num_witness_variables
        self.rows = cs.num_constraints()
        self.matrices = cs.to_matrices()[SR1CS_LABEL]
        self.z = cs.full_assignment()
        self.witness_col = [-1] * old_m
        self.instance_col = [-1] * old_m
        self.witness_col[0] = 0
        for m in (public_variables, witness_variables):
            for j, var in m.items():
                self.witness_col[j] = R.get_variable_index(var, self.ell)
        for k, j in enumerate(sorted(public_variables), start=1):          # BTreeMap::values(): ascending keys
            self.instance_col[j] = k


def adapter_reference(C, A, Bm, Cm, z, num_public) -> Adapted:
    """Sr1csAdapter::r1cs_to_sr1cs_with_assignment (sr1cs/mod.rs:191-265) on the matrices and the full assignment"""
    p = C.r
    new_cs = R.ConstraintSystem(p)
    del new_cs.predicates[R.R1CS_PREDICATE_LABEL]                         # :203 remove_predicate
    new_cs.register_predicate(SR1CS_LABEL, R.PredicateCS(R.PolynomialPredicate(p, 2, sr1cs_terms(p))))    # :204-207
    public_variables, witness_variables = {}, {}                          # :195-196

    def add_to_variable_maps_witness(constraint):                         # :85-116
        lc, val = [], 0
        for coeff, index in constraint:
            if index == 0:
                var, v = R.VAR_ONE, 1
            else:
                v = z[index]
                m = public_variables if index < num_public else witness_variables
                if index not in m:                                        # entry().or_insert_with(new_witness_variable)
                    m[index] = new_cs.new_witness_variable(lambda v=v: v)
                var = m[index]
            lc.append((coeff, var))
            val = (val + coeff * v) % p
        return lc, val

    for a_row, b_row, c_row in zip(A, Bm, Cm):                            # :213
        a_i, a_val = add_to_variable_maps_witness(a_row)
        b_i, b_val = add_to_variable_maps_witness(b_row)
        c_i, _ = add_to_variable_maps_witness(c_row)
        sq = (a_val - b_val) ** 2 % p
        square_variable = new_cs.new_witness_variable(lambda sq=sq: sq)   # :238
        c_i = [(4 * c % p, v) for c, v in c_i]                            # :241-243 double_in_place twice
        new_cs.enforce_constraint(SR1CS_LABEL, lambda: R.LC(p, a_i + b_i), lambda: R.LC(p, c_i + [(1, square_variable)]))
        new_cs.enforce_constraint(SR1CS_LABEL, lambda: R.LC(p, a_i + [((p - c) % p, v) for c, v in b_i]),
                                  lambda: R.LC(p, [(1, square_variable)]))
    for index in sorted(public_variables):                                # :253 values() of a BTreeMap
        old_var = public_variables[index]
        value = new_cs.assigned_value(old_var)
        new_var = new_cs.new_input_variable(lambda value=value: value)
        new_cs.enforce_constraint(SR1CS_LABEL, lambda: R.LC(p, [(1, old_var), (p - 1, new_var)]), lambda: R.LC(p))
    new_cs.finalize()                                                     # :263
    return Adapted(new_cs, public_variables, witness_variables, len(z))


def linear_forms(p, rows):
    """rows of (coeff, column) -> per row {column: summed coefficient}, zeros dropped"""
    out = []
    for row in rows:
        d = {}
        for c, j in row:
            d[j] = (d.get(j, 0) + c) % p
        out.append({j: c for j, c in d.items() if c})
    return out


def rows_from_csr(C, rp, col, coeff):
    cache = {}
    vals = []
    for e in range(len(col)):
        b = coeff[32 * e:32 * e + 32]
        v = cache.get(b)
        if v is None:
            v = cache[b] = Z.fr_from_mont(C, b)
        vals.append(v)
    return [[(vals[e], int(col[e])) for e in range(int(rp[i]), int(rp[i + 1]))] for i in range(len(rp) - 1)]


# ---- the device side ---------------------------------------------------------------------------------------------------------
def build(lib, ctx, C, A, Bm, Cm, ell, m, keep_r1cs=False):
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, m - ell)
    try:
        s = SR1CS.from_r1cs(lib, ctx, r1, C.curve_id, m)
    except Exception:
        lib.dll.ark355_r1cs_free(r1)
        raise
    if keep_r1cs:
        return s, r1
    lib.dll.ark355_r1cs_free(r1)              # the handle owns what it needs: everything below runs without the source
    return s, None


def assignment_dev(s, io, zb, m_in, m_out):
    d_z, k1 = io.to_dev(zb)
    d_out, k2 = io.alloc(m_out * 32)
    s.assignment_dev(d_z, m_in, d_out)
    return io.read(k2, m_out * 32)


def check_against_reference(lib, ctx, C, A, Bm, Cm, z, ell, io, ref=None):
    """every assertion of case 1: dims, var_map, both matrices as linear forms, assignment byte for byte, num_constraints,
    assignment_dev == assignment; returns the reference for the caller's own checks"""
    p, n, m = C.r, len(A), len(z)
    ref = ref or adapter_reference(C, A, Bm, Cm, z, ell)
    s, _ = build(lib, ctx, C, A, Bm, Cm, ell, m)
    try:
        n_ell, n_w, rows, nnz = s.dims
        assert (n_ell, n_w, rows) == (ref.ell, ref.w, ref.rows), ((n_ell, n_w, rows), (ref.ell, ref.w, ref.rows))
        P = n_ell - 1
        assert rows == 2 * n + P
        assert nnz == (2 * sum(len(r) for M in (A, Bm) for r in M) + 2 * P, sum(len(r) for r in Cm) + 2 * n)
        wit, inst = s.var_map()
        assert list(wit) == ref.witness_col, (list(wit), ref.witness_col)
        assert list(inst) == ref.instance_col, (list(inst), ref.instance_col)
        mats = s.matrices()
        for k in range(2):
            rp, col, coeff = mats[k]
            assert len(rp) == rows + 1 and int(rp[0]) == 0 and int(rp[-1]) == nnz[k] == len(col)
            assert all(int(rp[i]) <= int(rp[i + 1]) for i in range(rows))
            assert all(int(j) < n_ell + n_w for j in col)
            got = linear_forms(p, rows_from_csr(C, rp, col, coeff))
            want = linear_forms(p, ref.matrices[k])
            assert got == want, (C.name, k, [i for i in range(rows) if got[i] != want[i]][:5])
        zb = z_bytes(C, z)
        zp = s.assignment(zb)
        assert zp == z_bytes(C, ref.z), (C.name, "assignment")
        assert s.assignment(z) == zp                                     # canonical ints take the same route
        assert s.system.num_constraints() == ref.cs.num_constraints()
        assert assignment_dev(s, io, zb, m, n_ell + n_w) == zp
    finally:
        s.free()
    return ref


# ---- instances ---------------------------------------------------------------------------------------------------------------
def circuit2_instance(C):
    """the reference's circuit2 (gr1cs/tests/circuit2.rs:46-60) with a = 3, b = 5, c = 30"""
    cs = R.ConstraintSystem(C.r)
    R.circuit2(cs, 3, 5, 30)
    return S.cs_to_instance(cs)


def handmade_instance(C):
    """ell = 4 (One, x1, x2, x3), w = 5 (columns 4..8):
       x2 is used by nobody; column 6 first appears in B of row 0 and in A of row 2; column 7 occurs once, with coefficient
       zero; row 1 repeats column 5 inside A; row 3 has A == B (row 2i+1's left side cancels); x3 occurs only in C."""
    p = C.r
    A = [[(1, 4), (2, 1)], [(3, 5), (p - 1, 5), (1, 0)], [(1, 6), (5, 4)], [(7, 8), (1, 1)], []]
    Bm = [[(1, 6)], [(1, 4)], [(0, 7)], [(7, 8), (1, 1)], [(1, 0)]]
    Cm = [[(1, 5)], [(2, 0)], [(1, 3), (1, 5)], [(1, 4)], [(p - 3, 3), (1, 8)]]
    rnd = random.Random(0x5A11)
    z = [1] + [rnd.randrange(p) for _ in range(8)]
    return A, Bm, Cm, z, 4


def random_instance(C, n, seed, ell=None):
    """0-4 entries per row and matrix, each a coefficient of {0, 1, -1, random} times a random column; ell in 1..5"""
    p = C.r
    rnd = random.Random(seed)
    ell = rnd.randrange(1, 6) if ell is None else ell
    m = ell + max(3, n // 2)

    def row():
        return [(rnd.choice([0, 1, p - 1, rnd.randrange(p)]), rnd.randrange(m)) for _ in range(rnd.randrange(0, 5))]
    A, Bm, Cm = ([row() for _ in range(n)] for _ in range(3))
    z = [1] + [rnd.randrange(p) for _ in range(m - 1)]
    return A, Bm, Cm, z, ell


def same_columns_instance(C, n):
    """every row uses the same three columns: the first-occurrence atomics all land on them"""
    p = C.r
    rnd = random.Random(0x3C01)
    A = [[(rnd.randrange(1, p), 2)] for _ in range(n)]
    Bm = [[(1, 1), (rnd.randrange(1, p), 3)] for _ in range(n)]
    Cm = [[(p - 1, 3)] for _ in range(n)]
    return A, Bm, Cm, [1] + [rnd.randrange(p) for _ in range(4)], 2


# ---- 1 .. 3 ------------------------------------------------------------------------------------------------------------------
def reference_instances(C, dummy=16, bench=20):
    return [S.mulchain_direct(C.r, 13), S.cs_to_instance(S.dummy_cs(C.r, dummy)), S.cs_to_instance(S.bench_lc_cs(C.r, bench)),
            circuit2_instance(C), handmade_instance(C)]


def against_transliteration_case(lib, ctx, C, io, which):
    A, Bm, Cm, z, ell = reference_instances(C)[which]
    ref = check_against_reference(lib, ctx, C, A, Bm, Cm, z, ell, io)
    if which == 4:        # what the hand-made system is there for
        assert ref.instance_col[2] == -1 and ref.witness_col[2] == -1 and ref.ell == 3      # x2: no input at all
        assert ref.witness_col[7] >= 0                                                      # the zero coefficient counts
        assert ref.witness_col[6] < ref.witness_col[5]                                      # B of row 0 before C of row 0


def random_case(lib, ctx, C, io, n, seed):
    check_against_reference(lib, ctx, C, *random_instance(C, n, seed + C.curve_id), io)


def edges_case(lib, ctx, C, io, n_same=70):
    check_against_reference(lib, ctx, C, [], [], [], [1, 5, 6], 2, io)                      # n = 0: no rows, ell' = 1
    for seed in (1, 2, 3):
        check_against_reference(lib, ctx, C, *random_instance(C, 1, 0xE0 + seed), io)       # n = 1
    check_against_reference(lib, ctx, C, *random_instance(C, 40, 0xE11, ell=1), io)         # no publics
    check_against_reference(lib, ctx, C, *same_columns_instance(C, n_same), io)


# ---- 4: satisfaction transfer ------------------------------------------------------------------------------------------------
def satisfaction_case(lib, ctx, C, n):
    """mul-chain: (w_i + w_{i+1}) w_{i+1} = w_{i+2}, last row w_n * 1 = x_1"""
    p = C.r
    A, Bm, Cm, z, ell = S.mulchain_direct(p, n)
    m = len(z)
    s, r1 = build(lib, ctx, C, A, Bm, Cm, ell, m, keep_r1cs=True)
    try:
        n_ell, n_w, rows, _ = s.dims
        zs = [list(z), list(z), list(z)]
        zs[1][ell + 3] = (zs[1][ell + 3] + 1) % p              # w_3: C of row 1 (rows 2 and 3 read it as well)
        zs[2][1] = (zs[2][1] + 1) % p                          # x_1: the last row alone
        for k, (zz, want) in enumerate(zip(zs, (-1, 1, n - 1))):
            zb = z_bytes(C, zz)
            assert R.first_unsatisfied_r1cs(A, Bm, Cm, zz, p) == want
            first = lib.is_satisfied(ctx, r1, zb, m)
            assert first == want
            zp = s.assignment(zb)
            got = s.system.which_is_unsatisfied(zp)
            assert got == (None if first < 0 else (SR1CS_LABEL, 2 * first)), (C.name, k, got, first)
            ev = s.system.eval(SR1CS_LABEL, zp)
            res = [ev[32 * i:32 * i + 32] for i in range(rows)]
            zero = bytes(32)
            assert all(res[i] == zero for i in range(1, 2 * n, 2)), "an odd row is unsatisfied"
            assert all(res[i] == zero for i in range(2 * n, rows)), "an equality row is unsatisfied"
            bad_even = [i // 2 for i in range(0, 2 * n, 2) if res[i] != zero]
            assert bad_even == [i for i in range(n) if _row_fails(A, Bm, Cm, zz, i, p)]
    finally:
        lib.dll.ark355_r1cs_free(r1)
        s.free()


def _row_fails(A, Bm, Cm, z, i, p):
    dot = lambda row: sum(c * z[j] for c, j in row) % p        # noqa: E731
    return dot(A[i]) * dot(Bm[i]) % p != dot(Cm[i])


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------
def refusal_case(lib, ctx, C):
    A, Bm, Cm, z, ell = S.mulchain_direct(C.r, 5)
    m = len(z)
    r1 = r1cs_load_from_rows(lib, ctx, C, A, Bm, Cm, ell, m - ell)
    s = lib.sr1cs_from_r1cs(ctx, r1)
    d = lib.dll
    vp = ctypes.c_void_p
    try:
        n_ell, n_w, rows, nnz = lib.sr1cs_dims(s)
        zb = np.frombuffer(z_bytes(C, z), dtype=np.uint8).copy()
        out = np.zeros((n_ell + n_w) * 32, dtype=np.uint8)
        rp, col, cf = np.zeros(rows + 1, np.uint64), np.zeros(max(nnz), np.uint32), np.zeros(max(nnz) * 32, np.uint8)
        ptr = lambda a: a.ctypes.data_as(vp)                   # noqa: E731
        h = vp()

        def refused(rc, needle=None, code=B.EINVAL, message=True):
            assert rc == code, rc
            if message:
                msg = d.ark355_last_error(ctx).decode()
                assert msg and (needle is None or needle in msg), msg

        refused(d.ark355_sr1cs_from_r1cs(None, r1, ctypes.byref(h)), message=False)            # no context to carry a message
        refused(d.ark355_sr1cs_from_r1cs(ctx, None, ctypes.byref(h)), "r1cs is NULL")
        assert h.value is None
        refused(d.ark355_sr1cs_from_r1cs(ctx, r1, None), "out is NULL")
        assert d.ark355_sr1cs_system(None) is None
        d.ark355_sr1cs_free(None)
        refused(d.ark355_sr1cs_dims(None, None, None, None, None), message=False)
        assert d.ark355_sr1cs_dims(s, None, None, None, None) == 0                           # any pointer may be NULL
        refused(d.ark355_sr1cs_var_map(None, s, None, None), message=False)
        refused(d.ark355_sr1cs_var_map(ctx, None, None, None), "NULL")
        assert d.ark355_sr1cs_var_map(ctx, s, None, None) == 0                               # either may be NULL
        refused(d.ark355_sr1cs_matrix(None, s, 0, ptr(rp), ptr(col), ptr(cf), nnz[0]), message=False)
        refused(d.ark355_sr1cs_matrix(ctx, None, 0, ptr(rp), ptr(col), ptr(cf), nnz[0]), "NULL")
        refused(d.ark355_sr1cs_matrix(ctx, s, 0, None, ptr(col), ptr(cf), nnz[0]), "NULL")
        refused(d.ark355_sr1cs_matrix(ctx, s, 0, ptr(rp), None, ptr(cf), nnz[0]), "NULL")
        refused(d.ark355_sr1cs_matrix(ctx, s, 0, ptr(rp), ptr(col), None, nnz[0]), "NULL")
        refused(d.ark355_sr1cs_matrix(ctx, s, 2, ptr(rp), ptr(col), ptr(cf), nnz[0]), "which")
        refused(d.ark355_sr1cs_matrix(ctx, s, -1, ptr(rp), ptr(col), ptr(cf), nnz[0]), "which")
        for k in range(2):
            refused(d.ark355_sr1cs_matrix(ctx, s, k, ptr(rp), ptr(col), ptr(cf), nnz[k] - 1), "entry_capacity")
            assert d.ark355_sr1cs_matrix(ctx, s, k, ptr(rp), ptr(col), ptr(cf), nnz[k]) == 0
        for fn in (d.ark355_sr1cs_assignment, d.ark355_sr1cs_assignment_dev):
            refused(fn(None, s, ptr(zb), m, ptr(out)), message=False)
            refused(fn(ctx, None, ptr(zb), m, ptr(out)), "NULL")
            refused(fn(ctx, s, None, m, ptr(out)), "NULL")
            refused(fn(ctx, s, ptr(zb), m, None), "NULL")
            refused(fn(ctx, s, ptr(zb), m - 1, ptr(out)), "shorter", code=B.E_ASSIGNMENT_MISSING)
        # the borrowed system refuses what it cannot be: there is no "R1CS" predicate in it
        try:
            lib.dll.ark355_r1cs_free(lib.gr1cs_r1cs(ctx, lib.sr1cs_system(s)))
            assert False, "must refuse"
        except B.Ark355Error as e:
            assert e.code == B.EINVAL
        # the context and the handle stay usable
        assert lib.sr1cs_assignment(ctx, s, zb, m, n_ell + n_w, 32) == z_bytes(C, adapter_reference(C, A, Bm, Cm, z, ell).z)
    finally:
        lib.sr1cs_free(s)
        lib.dll.ark355_r1cs_free(r1)
