"""The h query in the evaluation basis (snark_amd/csrc/hbasis_impl.cuh, policy H_EVAL): cases shared by the CPU-emulator tier
(tests/test_emul_hbasis.py) and the GPU tier (tests/test_gpu_hbasis.py), through the C ABI, against the oracle.

References, computed once per process and shared:
  * group transforms: the DIRECT sums E'_j = sum_k c0 g^-k w^-jk H_k and U'_j = sum_k c0 w^-jk H_k (c0 = 1 / (N (g^N - 1))) with the
    Python oracle's curve arithmetic (`Group.msm`, naive).  At N = 2^6 that is 2 x 64 sums of 63 scalar multiplications per curve
    (a minute of Python): there every output is checked against the same sum taken in the exponent -- the inputs are H_k = s_k G
    with known s_k, so E'_j = (sum_k c0 g^-k w^-jk s_k) G, one fixed-base multiplication of the oracle per output -- and outputs
    0, 1, N/2 + 3 and N - 1 against the naive sum of points as well.
  * column gather: D_i = sum_j C[j][i] U_j, naive, same arithmetic.
  * proofs: the oracle's provers -- `prove_closed_form` (satisfied assignments), the seven-transform `prove` (the unsatisfied one),
    oracle/c (`cbase.prove`) where the Python generator would take too long.
"""
from __future__ import annotations

import json
import os
import random

import o3_cases as O
from helpers import ROOT, g1_vec_raw, pk_load_from_oracle, r1cs_load_from_rows, z_bytes
from oracle import groth16 as G, r1cs as R, serialize as Z, synthetic as S
from oracle.curves import g1
from oracle.ntt import Domain

_TRANSFORM_REF = {}
_POINTS = {}


def _g1_list(C, raw):
    sz = len(Z.g1_raw(C, None))
    return [Z.g1_from_raw(C, raw[i * sz:(i + 1) * sz]) for i in range(len(raw) // sz)]


def _points(C, count, seed):
    """`count` G1 points s_k G with their s_k (one fixed-base pass of the oracle per (curve, count, seed))"""
    k = (C.name, count, seed)
    if k not in _POINTS:
        rnd = random.Random(seed * 7919 + count)
        ss = [rnd.randrange(1, C.r) for _ in range(count)]
        G_ = g1(C)
        _POINTS[k] = (ss, G_.fixed_base_muls(G_.gen, ss))
    return _POINTS[k]


def transform_reference(C, log_n, inf_at=()):
    """(points H_k (N - 1), E' (N), U' (N), the few j whose outputs are ALSO the naive sums of points)"""
    key = (C.name, log_n, tuple(inf_at))
    if key in _TRANSFORM_REF:
        return _TRANSFORM_REF[key]
    G_ = g1(C)
    N = 1 << log_n
    d = Domain(C, log_n)
    ss, pts = _points(C, N - 1, 11 + log_n)
    ss, pts = list(ss), list(pts)
    for i in inf_at:
        ss[i], pts[i] = 0, None
    c0 = pow(N * (pow(d.g, N, C.r) - 1) % C.r, -1, C.r)

    def coeffs(j, shift):
        return [c0 * (pow(d.g_inv, k, C.r) if shift else 1) * pow(d.omega_inv, j * k, C.r) % C.r for k in range(N - 1)]

    naive_js = list(range(N)) if log_n <= 3 else [0, 1, N // 2 + 3, N - 1]
    exp = []
    for shift in (True, False):
        in_exponent = G_.fixed_base_muls(G_.gen, [sum(c * s for c, s in zip(coeffs(j, shift), ss)) % C.r for j in range(N)])
        for j in naive_js:
            assert G_.msm(pts, coeffs(j, shift)) == in_exponent[j], (C.name, log_n, j, shift)
        exp.append(in_exponent)
    _TRANSFORM_REF[key] = (pts, exp[0], exp[1], naive_js)
    return _TRANSFORM_REF[key]


def transform_case(lib, ctx, C, log_n, inf_at=()):
    pts, exp_e, exp_u, _ = transform_reference(C, log_n, inf_at)
    raw = g1_vec_raw(C, pts)
    e, u = lib.hbasis_transform(ctx, C.curve_id, raw, log_n)
    assert _g1_list(C, e) == exp_e, (C.name, log_n, "E'")
    assert _g1_list(C, u) == exp_u, (C.name, log_n, "U'")
    # each output alone (the entry point skips the copy of the scaled points then)
    assert lib.hbasis_transform(ctx, C.curve_id, raw, log_n, want_u=False)[0] == e
    assert lib.hbasis_transform(ctx, C.curve_id, raw, log_n, want_e=False)[1] == u


# ---- gather ---------------------------------------------------------------------------------------------------------------------
def hand_built_c(C):
    """(A, B, C, ell, w): five rows, two instance and four witness variables.  Columns of C: 0 (One) a non-unit coefficient,
    1 (the instance variable; the mulchain's last row has such an entry) two unit entries, 2 a unit entry and a -1, 3 two non-unit
    coefficients, 4 ONE unit entry, 5 empty."""
    r = C.r
    Cm = [[(1, 2), (1, 4)], [(5, 3), (r - 1, 2)], [(7, 3), (1, 1)], [(2, 0)], [(1, 1)]]
    A = [[(1, 2)], [(1, 3)], [(1, 4)], [(1, 5)], [(1, 2)]]
    B = [[(1, 0)]] * 5
    return A, B, Cm, 2, 4


def gather_expected(C, Cm, m, U):
    G_ = g1(C)
    cols = [[] for _ in range(m)]
    for j, row in enumerate(Cm):
        for c, i in row:
            cols[i].append((c, j))
    return [G_.msm([U[j] for _, j in col], [c for c, _ in col]) if col else None for col in cols]


def gather_hand_built_case(lib, ctx, C):
    A, B, Cm, ell, w = hand_built_c(C)
    m = ell + w
    r1 = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, w)
    try:
        N = lib.dll.ark355_r1cs_domain_size(r1)
        assert N == 8
        U = list(_points(C, N, 3)[1])
        U[1] = None                                  # a point at infinity among the inputs (row 1: columns 2 and 3)
        got = _g1_list(C, lib.hbasis_gather(ctx, r1, C.curve_id, g1_vec_raw(C, U), m))
        exp = gather_expected(C, Cm, m, U)
        assert exp[5] is None and exp[4] == U[0]
        assert got == exp
    finally:
        lib.dll.ark355_r1cs_free(r1)


def gather_heavy_case(lib, ctx, C, n):
    """The DummyCircuit: every entry of C sits in column 1 (an instance variable), n - 1 of them -- a heavy column, cut into chunks
    of 2048 entries (one workgroup each); every other column is empty."""
    n_, ell, w, mats, z = S.dummy_csr(C.r, n)
    r1 = lib.r1cs_load(ctx, C.curve_id, n_, ell, w, mats)
    try:
        N = lib.dll.ark355_r1cs_domain_size(r1)
        G_ = g1(C)
        # N points from a short list (the sum does not care): n - 1 of them enter
        base = _points(C, 64, 5)[1]
        U = [base[(j * 7 + j // 64) % 64] for j in range(N)]
        m = ell + w
        got = _g1_list(C, lib.hbasis_gather(ctx, r1, C.curve_id, g1_vec_raw(C, U), m))
        assert got[1] == G_.sum(U[:n - 1])
        assert all(p is None for i, p in enumerate(got) if i != 1)
    finally:
        lib.dll.ark355_r1cs_free(r1)


GATHER_LENGTHS = (2049, 63, 64, 65, 2048, 0)          # entries of columns 0 .. 5 of lengths_c: around the lane limit (64) and the chunk (2048)


def lengths_c(C):
    """(A, B, C, ell, w): 2049 rows, One and five witness variables.  Column i of C holds GATHER_LENGTHS[i] entries in distinct
    rows: 63 and 64 are summed by one lane, 65 is the shortest heavy column, 2048 fills one chunk, 2049 spills ONE entry into a
    second, column 5 is empty.  Unit coefficients but for seven: three in the 65-entry column (a lane of the chunk kernel
    multiplies) and four in the 2049-entry one, rows 0, 2047 and 2048 among them."""
    r = C.r
    n = max(GATHER_LENGTHS)
    rows_of = [[(7 * i + 5 * k) % n for k in range(ln)] for i, ln in enumerate(GATHER_LENGTHS)]     # 5 is prime to 2049 = 3 * 683
    assert all(len(set(rows)) == len(rows) for rows in rows_of)
    coeff = {(3, rows_of[3][0]): 5, (3, rows_of[3][31]): r - 1, (3, rows_of[3][64]): 7,
             (0, 0): 2, (0, 1000): r - 1, (0, 2047): 3, (0, 2048): 12345678901234567}
    Cm = [[] for _ in range(n)]
    for i, rows in enumerate(rows_of):
        for j in rows:
            Cm[j].append((coeff.get((i, j), 1), i))
    assert sum(c != 1 for row in Cm for c, _ in row) == len(coeff) <= 8
    A = [[(1, 1)]] * n
    B = [[(1, 0)]] * n
    return A, B, Cm, 1, 5


def gather_lengths_case(lib, ctx, C):
    A, B, Cm, ell, w = lengths_c(C)
    m = ell + w
    r1 = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, w)
    try:
        N = lib.dll.ark355_r1cs_domain_size(r1)
        assert N == 4096
        base = _points(C, 64, 5)[1]
        U = [base[(j * 7 + j // 64) % 64] for j in range(N)]
        U[9] = None                                  # a point at infinity among the inputs
        got = _g1_list(C, lib.hbasis_gather(ctx, r1, C.curve_id, g1_vec_raw(C, U), m))
        exp = gather_expected(C, Cm, m, U)
        assert exp[5] is None and all(p is not None for p in exp[:5])
        assert got == exp
    finally:
        lib.dll.ark355_r1cs_free(r1)


# ---- proofs ---------------------------------------------------------------------------------------------------------------------
TD = G.Trapdoor(tau=987654321, alpha=5, beta=7, gamma=11, delta=13)
RS = ((0x1234567890abcdef, 0xfedcba0987654321aabbccdd), (0, 0))          # and r = s = 0


def golden_circuit(C):
    """circuit2 of the reference's own test vectors (tests/golden/circuit2_matrices.json; coefficients 2 in C), with the assignment
    of the oracle's restatement of that circuit"""
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "circuit2_matrices.json")))["R1CS"]
    A, B, Cm = [[[(c, col) for c, col in row] for row in mat] for mat in raw]
    cs = R.ConstraintSystem(C.r)
    R.circuit2(cs, 1, 1, 2)
    cs.finalize()
    assert cs.to_matrices()[R.R1CS_PREDICATE_LABEL] == [A, B, Cm]
    return A, B, Cm, cs.full_assignment(), cs.num_instance_variables


def instance(C, name):
    if name.startswith("mulchain-"):
        return S.mulchain_direct(C.r, int(name.split("-")[1]))
    if name == "golden":
        return golden_circuit(C)
    if name == "ell1":
        # ONE instance variable (the constant): w0 w1 = w2, (w1 + 3) w2 = w3, w3 * 2 = 2 w3
        p = C.r
        w0, w1 = 1234567, 7654321
        w2 = w0 * w1 % p
        w3 = (w1 + 3) * w2 % p
        A = [[(1, 1)], [(1, 2), (3, 0)], [(1, 4)]]
        B = [[(1, 2)], [(1, 3)], [(2, 0)]]
        Cm = [[(1, 3)], [(1, 4)], [(2, 4)]]
        return A, B, Cm, [1, w0, w1, w2, w3], 1
    raise KeyError(name)


def prove_rows_case(lib, ctx, C, policy, name, h_eval, unsatisfied=False):
    """Key from the Python oracle's generator; policy H_EVAL forced to `h_eval`; the proof bytes of `ark355_prove` against the
    oracle's for (r, s) and for r = s = 0; the key must have settled on the path asked for."""
    A, B, Cm, z, ell = instance(C, name)
    m = len(z)
    sz = lib.sizes(C.curve_id)
    pk = G.setup(C, A, B, Cm, ell, m, TD)
    policy.setenv("ARK355_H_EVAL", str(h_eval))
    r1 = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, m - ell)
    pkh = pk_load_from_oracle(lib, ctx, C, pk, ell, m - ell, 1 << pk.domain_log)
    try:
        assert lib.pk_h_eval(pkh)["state"] == "undecided"
        if unsatisfied:
            z = list(z)
            z[ell + (m - ell) // 2] = (z[ell + (m - ell) // 2] + 1) % C.r
            assert R.first_unsatisfied_r1cs(A, B, Cm, z, C.r) is not None
            # rho_{N-1} != c_{N-1}: the top coefficient of a b - c does not vanish for this assignment
            d = Domain(C, pk.domain_log)
            n = len(A)
            ev = [R.mat_vec_mul(M, z, C.r) + [0] * (d.n - n) for M in (A, B, Cm)]
            for j in range(ell):
                ev[0][n + j] = z[j]
            a, b, c = (d.ifft(v) for v in ev)
            rho = d.coset_ifft([x * y % C.r for x, y in zip(d.coset_fft(a), d.coset_fft(b))])
            assert rho[d.n - 1] != c[d.n - 1]
        for r_, s_ in RS:
            r_, s_ = r_ % C.r, s_ % C.r
            a, b, c = lib.prove(ctx, pkh, r1, z_bytes(C, z), m, Z.fr_canon(C, r_), Z.fr_canon(C, s_), sz)
            got = G.Proof(Z.g1_from_raw(C, a), Z.g2_from_raw(C, b), Z.g1_from_raw(C, c))
            exp = G.prove(C, pk, A, B, Cm, z, ell, r_, s_) if unsatisfied else G.prove_closed_form(C, pk, z, ell, r_, s_)
            assert Z.proof_bytes(C, got) == Z.proof_bytes(C, exp), (C.name, name, h_eval, r_, s_)
        assert lib.pk_h_eval(pkh)["state"] == ("eval" if h_eval else "coeff")
    finally:
        lib.dll.ark355_pk_free(pkh)
        lib.dll.ark355_r1cs_free(r1)


def csr_instance(C, name):
    kind, n = name.split("-")
    return (S.mulchain_csr if kind == "mulchain" else S.dummy_csr)(C.r, int(n))


def prove_csr_case(lib, ctx, C, policy, name, h_eval, policy_value=None):
    """The same with the key and the expected proof from oracle/c (`cbase.setup_raw_c`, `cbase.prove`).  policy_value: what H_EVAL
    is set to when that is not `h_eval` itself (-1: the default rule, which must then settle on the path `h_eval` names)."""
    inst = csr_instance(C, name)
    n, ell, w, mats, z = inst
    pk = O.oracle_key(C, inst)
    zb = S._mont_bytes(C.r, z)
    sz = lib.sizes(C.curve_id)
    policy.setenv("ARK355_H_EVAL", str(h_eval if policy_value is None else policy_value))
    pkh, rh = O.load(lib, ctx, C, inst, pk)
    try:
        for r_, s_ in RS:
            r_, s_ = r_ % C.r, s_ % C.r
            got = lib.prove(ctx, pkh, rh, zb, len(z), Z.fr_canon(C, r_), Z.fr_canon(C, s_), sz)
            assert got == O.oracle_prove(C, inst, zb, pk, r_, s_), (C.name, name, h_eval, r_, s_)
        assert lib.pk_h_eval(pkh)["state"] == ("eval" if h_eval else "coeff")
    finally:
        O.free(lib, pkh, rh)


def check_satisfied_case(lib, ctx, C, policy):
    """Policy CHECK_SATISFIED on a key in the evaluation basis: the rows of C are still computed for the check."""
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 13)
    m = len(z)
    sz = lib.sizes(C.curve_id)
    pk = G.setup(C, A, B, Cm, ell, m, TD)
    policy.setenv("ARK355_H_EVAL", "1")
    policy.setenv("ARK355_CHECK_SATISFIED", "1")
    r1 = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, m - ell)
    pkh = pk_load_from_oracle(lib, ctx, C, pk, ell, m - ell, 1 << pk.domain_log)
    try:
        a, b, c = lib.prove(ctx, pkh, r1, z_bytes(C, z), m, Z.fr_canon(C, 77), Z.fr_canon(C, 99), sz)
        assert G.Proof(Z.g1_from_raw(C, a), Z.g2_from_raw(C, b), Z.g1_from_raw(C, c)) == G.prove_closed_form(C, pk, z, ell, 77, 99)
        assert lib.pk_h_eval(pkh)["state"] == "eval"
        zbad = list(z)
        zbad[ell + 6] = (zbad[ell + 6] + 1) % C.r
        bad = R.first_unsatisfied_r1cs(A, B, Cm, zbad, C.r)
        try:
            lib.prove(ctx, pkh, r1, z_bytes(C, zbad), m, Z.fr_canon(C, 77), Z.fr_canon(C, 99), sz)
            assert False, "unsatisfied assignment must be refused under CHECK_SATISFIED"
        except Exception as e:
            assert getattr(e, "code", None) == -17, e
            assert ("constraint %d " % bad) in str(e)
    finally:
        lib.dll.ark355_pk_free(pkh)
        lib.dll.ark355_r1cs_free(r1)


def other_r1cs_refused_case(lib, ctx, C, policy):
    """A key in the evaluation basis is bound to the R1CS handle of its first proof: another handle (even of equal matrices) is
    answered with ARK355_EINVAL, the first one keeps proving; a key on the coefficient path takes any handle of its dimensions."""
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 6)
    m = len(z)
    sz = lib.sizes(C.curve_id)
    pk = G.setup(C, A, B, Cm, ell, m, TD)
    exp = Z.proof_bytes(C, G.prove_closed_form(C, pk, z, ell, 3, 4))

    def prove(pkh, r1):
        a, b, c = lib.prove(ctx, pkh, r1, z_bytes(C, z), m, Z.fr_canon(C, 3), Z.fr_canon(C, 4), sz)
        return Z.proof_bytes(C, G.Proof(Z.g1_from_raw(C, a), Z.g2_from_raw(C, b), Z.g1_from_raw(C, c)))

    r1a = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, m - ell)
    r1b = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, m - ell)
    try:
        for h_eval in (1, 0):
            policy.setenv("ARK355_H_EVAL", str(h_eval))
            pkh = pk_load_from_oracle(lib, ctx, C, pk, ell, m - ell, 1 << pk.domain_log)
            try:
                assert prove(pkh, r1a) == exp
                if h_eval:
                    try:
                        prove(pkh, r1b)
                        assert False, "a bound key must refuse another R1CS handle"
                    except Exception as e:
                        assert getattr(e, "code", None) == -1, e
                else:
                    assert prove(pkh, r1b) == exp
                assert prove(pkh, r1a) == exp
            finally:
                lib.dll.ark355_pk_free(pkh)
    finally:
        lib.dll.ark355_r1cs_free(r1a)
        lib.dll.ark355_r1cs_free(r1b)


def sharded_key_case(lib, ctx, C, policy):
    """Key shards keep the coefficient path whatever H_EVAL says: two shards of one key, policy forced to 1, settle on 'coeff' at
    load time; their partial sums combine to the oracle's proof."""
    A, B, Cm, z, ell = S.mulchain_direct(C.r, 13)
    m = len(z)
    sz = lib.sizes(C.curve_id)
    pk = G.setup(C, A, B, Cm, ell, m, TD)
    policy.setenv("ARK355_H_EVAL", "1")
    r1 = r1cs_load_from_rows(lib, ctx, C, A, B, Cm, ell, m - ell)
    args = (g1_vec_raw(C, pk.a_query), g1_vec_raw(C, pk.b_g1_query), b"".join(Z.g2_raw(C, p) for p in pk.b_g2_query),
            g1_vec_raw(C, pk.h_query), g1_vec_raw(C, pk.l_query), Z.g1_raw(C, pk.vk.alpha_g1), Z.g1_raw(C, pk.beta_g1),
            Z.g1_raw(C, pk.delta_g1), Z.g2_raw(C, pk.vk.beta_g2), Z.g2_raw(C, pk.vk.delta_g2))
    shards = [lib.pk_load(ctx, C.curve_id, ell, m - ell, 1 << pk.domain_log, *args, shard=(k, 2)) for k in range(2)]
    try:
        assert [lib.pk_h_eval(h)["state"] for h in shards] == ["coeff", "coeff"]
        r_, s_ = 77, 99
        parts = b"".join(lib.prove_shard(ctx, C.curve_id, h, r1, z_bytes(C, z), m, Z.fr_canon(C, r_), Z.fr_canon(C, s_)) for h in shards)
        a, b, c = lib.prove_combine(ctx, C.curve_id, parts, 2, Z.fr_canon(C, r_), Z.fr_canon(C, s_), sz)
        got = G.Proof(Z.g1_from_raw(C, a), Z.g2_from_raw(C, b), Z.g1_from_raw(C, c))
        assert Z.proof_bytes(C, got) == Z.proof_bytes(C, G.prove_closed_form(C, pk, z, ell, r_, s_))
        assert [lib.pk_h_eval(h) for h in shards] == [{"state": "coeff", "binds": 0, "bind_seconds": 0.0}] * 2
    finally:
        for h in shards:
            lib.dll.ark355_pk_free(h)
        lib.dll.ark355_r1cs_free(r1)


def concurrent_first_proofs_case(lib, ctx, C, n):
    """Two contexts whose first proofs on one fresh key start together, under the context's own H_EVAL (the default at n = 2^16 - 2:
    N = 2^16 is the smallest domain that moves to the evaluation basis by itself): both proofs equal oracle/c's, the key was
    converted once."""
    import threading
    inst = S.mulchain_csr(C.r, n)
    n_, ell, w, mats, z = inst
    pk = O.oracle_key(C, inst)
    zb = S._mont_bytes(C.r, z)
    sz = lib.sizes(C.curve_id)
    rs = [(0x1234567, 0x89ABCDE), (77, C.r - 2)]
    exp = [O.oracle_prove(C, inst, zb, pk, r_, s_) for r_, s_ in rs]
    pkh, rh = O.load(lib, ctx, C, inst, pk)
    ctx2 = lib.ctx_create(0)
    got, errs = [None, None], []
    start = threading.Barrier(2)

    def work(k, c):
        try:
            start.wait()
            got[k] = lib.prove(c, pkh, rh, zb, len(z), Z.fr_canon(C, rs[k][0]), Z.fr_canon(C, rs[k][1]), sz)
        except Exception as e:                   # noqa: BLE001 -- reported by the assertion below
            errs.append(e)

    try:
        assert lib.pk_h_eval(pkh)["state"] == "undecided"
        th = [threading.Thread(target=work, args=(k, c)) for k, c in enumerate((ctx, ctx2))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        assert got == exp
        info = lib.pk_h_eval(pkh)
        assert info["state"] == "eval" and info["binds"] == 1 and info["bind_seconds"] > 0, info
        return info
    finally:
        lib.ctx_destroy(ctx2)
        O.free(lib, pkh, rh)
