"""Cases of the multilinear openings, shared by the CPU-emulator tier and the GPU tier (tests/test_emul_mle_open.py,
tests/test_gpu_mle_open.py): ark355_mle_quotients_fr, its `_dev` variant and ark355_mle_open_dev (include/ark355.h "Multilinear
openings").  Every comparison is byte for byte or an exact identity of integers.

The reference is plain big-integer code: quot_ref folds a table with fold_ref of tests/sumcheck_cases.py and keeps the differences
q_j[i] = f^(j)[2i+1] - f^(j)[2i]; layout_ref places them as the header says (level j at N - 2^(v-j), the value at N - 1).  The group
side is oracle.curves: a proof element is [q_j~(t_{j+1} .. t_{v-1})] base for the trapdoor t the key was made from.

The quotients are linear in the table, so they are compared on raw Montgomery images (v R mod r) with the canonical point, as
tests/sumcheck_cases.py compares fix / eval; the openings need the real values and go through real conversions.

The `_dev` variants always write into buffers pre-filled with 0xA5 that are one element longer than needed, and the extra element
is checked after every call.  `io` carries the tier's device memory, as in tests/sr1cs_cases.py.  Not reachable at a test's size,
and so not covered: ARK355_ENOMEM."""
from __future__ import annotations

import ctypes
import random

import numpy as np

import evals_cases as ec
import gr1cs_cases as gc
import poly_cases as pc
import quotient_cases as qc
import sumcheck_cases as sk
from helpers import z_bytes
from oracle import curves as OC
from oracle import serialize as Z
from oracle.fields import BLS12_381, BN254
from snark_amd import _binding as B
from snark_amd.poly import Mle

POLICY = "ARK355_MLE_OPEN_LANE_ENTRIES"
E_DEFAULT = 8
MAX_COUNT = 1024
A5 = b"\xA5" * 32
# A lane owns E entries, a wave 64 E, a workgroup K = 256 E, a pass log2 K halvings.
# E = 8: inside a lane and at its border (v = 0 .. 4), the wave border at 2^9 (8, 9, 10), one full workgroup (11), a second pass of
# 2, 4 and 8 entries (12, 13, 14).  E = 2: the lane (1, 2), the wave border at 2^7 (6, 7, 8), the workgroup (9), a second pass (10, 11).
# E = 1: no register halving at all (0, 1), the wave border at 2^6 (7), the workgroup at 2^8 (8), a second pass (9).
SHAPES_E8 = (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13, 14)
SHAPES_E2 = (1, 2, 6, 7, 8, 9, 10, 11)
SHAPES_E1 = (0, 1, 7, 8, 9)
THIRD_PASS = ((1, 17), (2, 19))               # (E, v): 2^17 = 256^2 * 2, 2^19 = 512^2 * 2

xb, raw, unraw, expect_refusal = pc.xb, pc.raw, pc.unraw, pc.expect_refusal
mont, fr_list = qc.mont, qc.fr_list
fold_ref, eval_def, point_bytes = sk.fold_ref, sk.eval_def, sk.point_bytes
level = Mle.level


# ---- the reference: plain integers -----------------------------------------------------------------------------------------------
def quot_ref(p, f, point):
    """([q_0, .., q_{v-1}], f~(point)) by the header's recurrence"""
    levels = []
    for r in point:
        levels.append([(f[2 * i + 1] - f[2 * i]) % p for i in range(len(f) // 2)])
        f = fold_ref(p, f, r)
    return levels, f[0] % p


def layout_ref(p, tables, point):
    """(the count x N output as integers, the values)"""
    out, vals = [], []
    for f in tables:
        levels, y = quot_ref(p, f, point)
        out += [x for q in levels for x in q] + [y]
        vals.append(y)
    return out, vals


def check_layout(v):
    """the level helper against the header's sentence: back to back, largest first, N - 1 left for the value"""
    N, at = 1 << v, 0
    for j in range(v):
        assert level(v, j) == (at, N >> (j + 1)) and at == N - (1 << (v - j))
        at += N >> (j + 1)
    assert at == N - 1


# ---- quotients -------------------------------------------------------------------------------------------------------------------
def dev_quot(lib, ctx, C, io, fb, v, count, point, want_rem=True):
    size = (count << v) * 32
    d_f, k0 = io.to_dev(fb + A5)
    d_q, k1 = io.alloc(size + 32)
    d_r, k2 = io.alloc(count * 32 + 32)
    lib.mle_quotients_fr_dev(ctx, C.curve_id, d_f, v, count, point_bytes(point), d_q, d_r if want_rem else None)
    got, rem = io.read(k1, size + 32), io.read(k2, count * 32 + 32)
    assert got[size:] == A5, "quotients wrote behind q_out"
    assert rem[count * 32:] == A5 and (want_rem or rem[:32] == A5), "quotients wrote behind rem_out, or into a rem_out it did not get"
    assert io.read(k0, len(fb) + 32) == fb + A5, "quotients changed their input"
    return got[:size], (rem[:count * 32] if want_rem else None)


def tables_of(C, rnd, N, count):
    """name -> count x N raw images: random; constant (every quotient zero); the indicator of one index; every entry r - 1"""
    p = C.r
    out = {"random": [rnd.randrange(p) for _ in range(count * N)]}
    out["constant"] = [c for _ in range(count) for c in [rnd.randrange(1, p)] * N]
    hot = [rnd.randrange(N) for _ in range(count)]
    out["indicator"] = [int(i == hot[c]) * (c + 1) for c in range(count) for i in range(N)]
    out["r-1"] = [p - 1] * (count * N)
    return out


def quotients_case(lib, ctx, C, io, policy, E, v, counts=(1, 3)):
    """host and `_dev` variants against layout_ref; the value against ark355_mle_eval_fr; the levels against the differences of
    ark355_mle_fix_fr's output; the defining identity at three random X"""
    p = C.r
    policy.setenv(POLICY, E)
    check_layout(v)
    rnd = random.Random("mle-open/%d/%d/%d" % (v, E, C.curve_id))
    N = 1 << v
    pts = sk.mle_points(C, rnd, v)
    mle = Mle(C.name, lib=lib, ctx=ctx)
    for count in counts:
        tabs = tables_of(C, rnd, N, count)
        # every point on the random tables, every table at the random and the mixed point
        pairs = [(pn, "random") for pn in pts] + [(pn, tn) for pn in ("random", "mixed") for tn in tabs if tn != "random"]
        if count != counts[0]:
            pairs = [("random", "random"), ("mixed", "r-1"), ("boolean", "indicator")]
        for pn, tn in pairs:
            point, f = pts[pn], tabs[tn]
            tag = (C.name, v, E, count, pn, tn)
            fb = unraw(f)
            tables = [f[c * N:(c + 1) * N] for c in range(count)]
            want, vals = layout_ref(p, tables, point)
            wb = unraw(want)
            q, rem = dev_quot(lib, ctx, C, io, fb, v, count, point)
            assert q == wb, (tag, "quotients_dev", qc.first_difference(q, wb))
            assert rem == unraw(vals), (tag, "rem_out")
            assert rem == lib.mle_eval_fr(ctx, C.curve_id, fb, v, count, point_bytes(point)), (tag, "the value is not mle_eval_fr's")
            if tn == "constant":
                assert all(not any(q[(c * N) * 32:(c * N + N - 1) * 32]) for c in range(count)), (tag, "a constant table has a quotient")
            if pn == "random" or tn != "random":
                assert mle.quotients(fb, v, point, count) == (q, rem), (tag, "host form")
            if (pn, tn) == ("random", "random"):
                assert dev_quot(lib, ctx, C, io, fb, v, count, point, want_rem=False)[0] == q, (tag, "without rem_out")
                assert mle.quotients(fb, v, point, count, want_rem=False) == (q, None), (tag, "host form without rem_out")
                for j in sorted(set(range(v) if v <= 9 else (0, 1, v // 2, v - 1))):       # level j from fix(k = j)
                    g = raw(lib.mle_fix_fr(ctx, C.curve_id, fb, v, count, point_bytes(point[:j]), j))
                    M = N >> j
                    off, ln = level(v, j)
                    for c in range(count):
                        diff = unraw((g[c * M + 2 * i + 1] - g[c * M + 2 * i]) % p for i in range(M // 2))
                        assert q[(c * N + off) * 32:(c * N + off + ln) * 32] == diff, (tag, "level %d against fix" % j)
                for _ in range(3):                                                          # the defining identity, through eval
                    X = [rnd.randrange(p) for _ in range(v)]
                    for c in range(count):
                        lhs = (raw(lib.mle_eval_fr(ctx, C.curve_id, unraw(tables[c]), v, 1, point_bytes(X)))[0] - vals[c]) % p
                        rhs = 0
                        for j in range(v):
                            off, ln = level(v, j)
                            row = q[(c * N + off) * 32:(c * N + off + ln) * 32]
                            rhs += (X[j] - point[j]) * raw(lib.mle_eval_fr(ctx, C.curve_id, row, v - 1 - j, 1, point_bytes(X[j + 1:])))[0]
                        assert lhs == rhs % p, (tag, "f~(X) - f~(p) != sum_j (X_j - p_j) q_j~")
    policy.setenv(POLICY, E_DEFAULT)


def third_pass_case(lib, ctx, C, io, policy, E, v):
    """a table of 256 E x 256 E x 2 entries: the third pass holds one pair; against the full reference"""
    p = C.r
    policy.setenv(POLICY, E)
    rnd = random.Random("mle-open/third/%d/%d/%d" % (v, E, C.curve_id))
    N = 1 << v
    f = [rnd.getrandbits(250) % p for _ in range(N)]
    point = [rnd.randrange(p) for _ in range(v)]
    want, vals = layout_ref(p, [f], point)
    q, rem = dev_quot(lib, ctx, C, io, unraw(f), v, 1, point)
    assert q == unraw(want), (C.name, v, E, qc.first_difference(q, unraw(want)))
    assert rem == unraw(vals)
    policy.setenv(POLICY, E_DEFAULT)


def policy_case(lib, ctx, C, io, policy, v=9):
    """every value from -3 to 100 leaves every byte unchanged"""
    p = C.r
    rnd = random.Random("mle-open/policy/%d" % C.curve_id)
    count, N = 2, 1 << v
    f = [rnd.randrange(p) for _ in range(count * N)]
    point = [rnd.randrange(p) for _ in range(v)]
    want, vals = layout_ref(p, [f[:N], f[N:]], point)
    for value in [E_DEFAULT] + list(range(-3, 101)):
        policy.setenv(POLICY, value)
        assert dev_quot(lib, ctx, C, io, unraw(f), v, count, point) == (unraw(want), unraw(vals)), \
            (C.name, "MLE_OPEN_LANE_ENTRIES = %d changed the bytes" % value)
    policy.setenv(POLICY, E_DEFAULT)


# ---- openings --------------------------------------------------------------------------------------------------------------------
class Key:
    """the PST key of Mle.commit_key over a known trapdoor, and the oracle's side of the same group"""

    def __init__(self, lib, ctx, C, io, group, t):
        self.lib, self.ctx, self.C, self.group, self.t = lib, ctx, C, group, list(t)
        self.G = OC.g1(C) if group == 1 else OC.g2(C)
        self.gen = C.g1_gen if group == 1 else C.g2_gen
        self.enc = Z.g1_raw if group == 1 else Z.g2_raw
        self.size = lib.sizes(C.curve_id)["g1" if group == 1 else "g2"]
        self.mle = Mle(C.name, lib=lib, ctx=ctx)
        self.commit, self.levels = self.mle.commit_key(group, self.enc(C, self.gen), self.t, alloc=io.alloc)

    def point_of(self, scalar):
        """[scalar] base by the oracle, in the library's bytes"""
        return self.enc(self.C, self.G.mul(self.gen, scalar % self.C.r) if scalar % self.C.r else None)

    def free(self):
        for h in [self.commit] + self.levels:
            self.lib.dll.ark355_bases_free(h)


def open_scalars(p, f, point, t):
    """(q_j~(t_{j+1} .. t_{v-1}) for every j, f~(point)): what the proof elements are multiples of"""
    levels, y = quot_ref(p, f, point)
    return [eval_def(p, q, t[j + 1:]) for j, q in enumerate(levels)], y


def open_tables(C, rnd, v):
    p, N = C.r, 1 << v
    return {"random": [rnd.randrange(p) for _ in range(N)], "constant": [rnd.randrange(1, p)] * N}


def check_open(key, io, f, point, tag):
    """open_dev against the oracle, against ark355_msm_dev on the rows of quotients_dev, and the identity the verifier relies on"""
    lib, ctx, C = key.lib, key.ctx, key.C
    p, v = C.r, len(point)
    N = 1 << v
    fb = mont(C, f)
    d_f, k0 = io.to_dev(fb + A5)
    proofs, value = key.mle.open_dev(key.levels, d_f, v, point, key.group)
    assert io.read(k0, len(fb) + 32) == fb + A5, (tag, "open_dev changed its input")
    scalars, y = open_scalars(p, f, point, key.t)
    assert value == mont(C, [y]), (tag, "value_out")
    assert len(proofs) == v * key.size
    assert sum((key.t[j] - point[j]) * s for j, s in enumerate(scalars)) % p == (eval_def(p, f, key.t) - y) % p, (tag, "the reference itself")
    d_q, k1 = io.alloc((N + 1) * 32)
    lib.mle_quotients_fr_dev(ctx, C.curve_id, d_f, v, 1, point_bytes(point), d_q, None)
    for j in range(v):
        pi = proofs[j * key.size:(j + 1) * key.size]
        assert pi == key.point_of(scalars[j]), (tag, "proof element %d against the oracle" % j)
        off, ln = level(v, j)
        assert pi == lib.msm_dev(ctx, key.levels[j], d_q + off * 32, ln, 1, key.size), (tag, "proof element %d against msm_dev" % j)
    return proofs, value


def open_case(lib, ctx, C, io, group, v):
    p = C.r
    rnd = random.Random("mle-open/open/%d/%d/%d" % (group, v, C.curve_id))
    key = Key(lib, ctx, C, io, group, [rnd.randrange(1, p) for _ in range(v)])
    try:
        for tn, f in open_tables(C, rnd, v).items():
            point = [rnd.randrange(p) for _ in range(v)]
            proofs, value = check_open(key, io, f, point, (C.name, group, v, tn))
            if tn == "constant":
                assert not any(proofs) and value == mont(C, f[:1]), (C.name, group, v, "a constant table opens to v points at infinity")
        if v >= 2:                                               # one level zero, the others not: f depends on variable 1 alone
            a, b = rnd.randrange(p), rnd.randrange(p)
            f = [(a, b)[(i >> 1) & 1] for i in range(1 << v)]
            proofs, _ = check_open(key, io, f, [rnd.randrange(p) for _ in range(v)], (C.name, group, v, "variable 1 alone"))
            assert [any(proofs[j * key.size:(j + 1) * key.size]) for j in range(v)] == [j == 1 for j in range(v)]
    finally:
        key.free()


def pairing_case(lib, ctx, C, io, v=6):
    """the verifier's check with G1 proofs: e(C - [y] g, -h) prod_j e(pi_j, [t_j - p_j] h) = 1, and not after one proof element or
    the value is altered"""
    p = C.r
    rnd = random.Random("mle-open/pairing/%d" % C.curve_id)
    t = [rnd.randrange(1, p) for _ in range(v)]
    key = Key(lib, ctx, C, io, 1, t)
    try:
        G1, G2 = OC.g1(C), OC.g2(C)
        f = [rnd.randrange(p) for _ in range(1 << v)]
        point = [rnd.randrange(p) for _ in range(v)]
        d_f, k0 = io.to_dev(mont(C, f))
        com = lib.msm_dev(ctx, key.commit, d_f, 1 << v, 1, key.size)
        assert com == key.point_of(eval_def(p, f, t)), (C.name, "the commitment is not [f~(t)] g")
        proofs, value = key.mle.open_dev(key.levels, d_f, v, point, 1)
        y = Z.fr_from_mont(C, value)
        h2 = b"".join(Z.g2_raw(C, G2.mul(C.g2_gen, (t[j] - point[j]) % p)) for j in range(v))
        minus_h = Z.g2_raw(C, G2.neg(C.g2_gen))

        def product_is_one(proofs, y):
            lhs = G1.add(Z.g1_from_raw(C, com), G1.neg(G1.mul(C.g1_gen, y)) if y else None)
            return lib.multi_pairing(ctx, C.curve_id, Z.g1_raw(C, lhs) + proofs, minus_h + h2, v + 1, want_gt=False)[1]

        assert product_is_one(proofs, y), (C.name, "the pairing product of an honest opening is not 1")
        assert not product_is_one(proofs, (y + 1) % p), (C.name, "the pairing product accepts another value")
        bad = Z.g1_raw(C, G1.add(Z.g1_from_raw(C, proofs[2 * key.size:3 * key.size]), C.g1_gen))
        assert not product_is_one(proofs[:2 * key.size] + bad + proofs[3 * key.size:], y), (C.name, "an altered proof element is accepted")
    finally:
        key.free()


def chain_case(lib, ctx, C, io, name="circuit2"):
    """a resident system: ark355_gr1cs_mat_vec_dev -> sum-check with challenges -> open_dev of table 0 at the final point; the value
    is finals_out[0] and the proof is the oracle's"""
    p = C.r
    ell, w, spec, z, col = qc.satisfied_systems(C)[name]
    rnd = random.Random("mle-open/chain/%s/%d" % (name, C.curve_id))
    g = gc.load(lib, ctx, C, ell, w, spec)
    key = None
    try:
        label = next(iter(spec))
        arity, terms, mats = spec[label]
        v = g.quotient_dims(label)[1]
        d_z, k_z = io.to_dev(z_bytes(C, z))
        d_t, k_t, N, vecs = ec.mat_vec_dev(g, io, label, d_z, len(z), len(mats[0]))
        assert N == 1 << v
        challenges = [rnd.randrange(p) for _ in range(v)]
        with g.sumcheck_dev(label, d_t, None, v) as sc:
            for j in range(v):
                sc.round(challenges[j - 1] if j else None)
            finals = sc.finish(challenges[-1])
        key = Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(v)])
        proofs, value = check_open(key, io, fr_list(C, vecs[0]), challenges, (C.name, name, "chain"))
        proofs_dev, value_dev = key.mle.open_dev(key.levels, d_t, v, challenges, 1)      # the resident table itself
        assert (proofs_dev, value_dev) == (proofs, value)
        assert value == finals[:32], (C.name, name, "value_out is not finals_out[0]")
    finally:
        if key:
            key.free()
        g.free()


# ---- robustness ------------------------------------------------------------------------------------------------------------------
def dirty_sequence(lib, ctx, C, io):
    """in a fresh context: a large open, a small open, an MSM of another size, small quotients with other data, the large open again;
    every step against the reference"""
    p = C.r
    rnd = random.Random("mle-open/dirty/%d" % C.curve_id)
    big, small = 6, 2
    kb = Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(big)])
    ks = Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(small)])
    try:
        fbig, pbig = [rnd.randrange(p) for _ in range(1 << big)], [rnd.randrange(p) for _ in range(big)]
        first = check_open(kb, io, fbig, pbig, (C.name, "large open"))
        check_open(ks, io, [rnd.randrange(p) for _ in range(1 << small)], [rnd.randrange(p) for _ in range(small)], (C.name, "small open"))
        s = [rnd.randrange(p) for _ in range(23)]
        d_s, k = io.to_dev(mont(C, s))
        eq_t = sk.eq_ref(p, kb.t)
        assert lib.msm_dev(ctx, kb.commit, d_s, 23, 1, kb.size) == kb.point_of(sum(a * b for a, b in zip(s, eq_t))), (C.name, "MSM of 23")
        f = [rnd.randrange(p) for _ in range(3 << 3)]
        pt = [rnd.randrange(p) for _ in range(3)]
        want, vals = layout_ref(p, [f[c * 8:(c + 1) * 8] for c in range(3)], pt)
        assert dev_quot(lib, ctx, C, io, unraw(f), 3, 3, pt) == (unraw(want), unraw(vals)), (C.name, "small quotients")
        expect_refusal(lib, ctx, lambda: lib.mle_quotients_fr(ctx, C.curve_id, unraw(f), 3, 3, point_bytes([1, p, 2])), needle="point[1]")
        assert check_open(kb, io, fbig, pbig, (C.name, "large open again")) == first
    finally:
        kb.free()
        ks.free()


def interleaved_case(lib, ctx, C, io, v=5):
    """ark355_msm_dev and ark355_mle_fix_fr_dev between two opens: unchanged bytes (the quotients keep their own scratch)"""
    p = C.r
    rnd = random.Random("mle-open/interleaved/%d" % C.curve_id)
    key = Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(v)])
    try:
        f, point = [rnd.randrange(p) for _ in range(1 << v)], [rnd.randrange(p) for _ in range(v)]
        d_f, k0 = io.to_dev(mont(C, f))
        first = key.mle.open_dev(key.levels, d_f, v, point, 1)
        other = [rnd.randrange(p) for _ in range(1 << 10)]
        d_o, k1 = io.to_dev(mont(C, other))
        com = lib.msm_dev(ctx, key.commit, d_o, 1 << v, 1, key.size)
        assert com == key.point_of(eval_def(p, other[:1 << v], key.t))
        fixed = sk.dev_fix(lib, ctx, C, io, unraw(other), 10, 1, [rnd.randrange(p) for _ in range(4)])
        assert len(fixed) == 32 << 6
        assert key.mle.open_dev(key.levels, d_f, v, point, 1) == first, (C.name, "other entries between two opens changed the bytes")
        assert first[1] == mont(C, [eval_def(p, f, point)])
    finally:
        key.free()


def overlap_case(lib, ctx, C, io, v=4, count=2):
    """every overlap of q_out with evals, and of rem_out with either, down to one element; nothing is written"""
    p = C.r
    rnd = random.Random("mle-open/overlap/%d" % C.curve_id)
    n = count << v
    size = n * 32
    fb = unraw(rnd.randrange(p) for _ in range(n))
    point = [rnd.randrange(p) for _ in range(v)]
    pb = point_bytes(point)
    whole = A5 * n + fb + A5 * n
    d_b, keep = io.to_dev(whole)
    d_c = d_b + size
    for d_q in (d_c, d_c + 32, d_c - 32, d_c + size - 32, d_c - size + 32):
        expect_refusal(lib, ctx, lambda: lib.mle_quotients_fr_dev(ctx, C.curve_id, d_c, v, count, pb, d_q, None), needle="overlap")
    for d_r in (d_c, d_c + size - 32, d_c - (count - 1) * 32, d_b, d_b + size - 32, d_b - (count - 1) * 32):   # q_out = d_b
        expect_refusal(lib, ctx, lambda: lib.mle_quotients_fr_dev(ctx, C.curve_id, d_c, v, count, pb, d_b, d_r), needle="overlap")
    assert io.read(keep, 3 * size) == whole, "a refused call wrote"
    lib.mle_quotients_fr_dev(ctx, C.curve_id, d_c, v, count, pb, d_b, d_c + size)           # touching is not overlapping
    got = io.read(keep, 3 * size)
    want, vals = layout_ref(p, [raw(fb)[c << v:(c + 1) << v] for c in range(count)], point)
    assert got == unraw(want) + fb + unraw(vals) + A5 * (n - count)


def refusals_case(lib, ctx, C, io):
    """every refusal a test's size reaches, each by code and with a message, each followed by a good call on the same context"""
    p = C.r
    d = lib.dll
    vp = ctypes.c_void_p
    ptr = lambda a: a.ctypes.data_as(vp)                       # noqa: E731
    rnd = random.Random(0x0BE4 + C.curve_id)
    v, count = 3, 2
    f = [rnd.randrange(p) for _ in range(count << v)]
    fb = unraw(f)
    c = np.frombuffer(fb, dtype=np.uint8).copy()
    out = np.zeros(32 * 64, dtype=np.uint8)
    rem = np.zeros(32 * 4, dtype=np.uint8)
    point = [rnd.randrange(p) for _ in range(v)]
    pt = np.frombuffer(point_bytes(point), dtype=np.uint8).copy()
    pt_r = np.frombuffer(point_bytes(point[:1] + [p] + point[2:]), dtype=np.uint8).copy()
    want, vals = layout_ref(p, [f[:1 << v], f[1 << v:]], point)

    def good():
        assert lib.mle_quotients_fr(ctx, C.curve_id, fb, v, count, point_bytes(point)) == (unraw(want), unraw(vals))

    def refused(rc, needle=None, code=B.EINVAL, message=True):
        assert rc == code, rc
        if message:
            msg = d.ark355_last_error(ctx).decode()
            assert msg and (needle is None or needle in msg), msg
            good()

    for fn in (d.ark355_mle_quotients_fr, d.ark355_mle_quotients_fr_dev):
        refused(fn(ctx, C.curve_id, None, v, count, ptr(pt), ptr(out), None), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, None, ptr(out), None), "NULL")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), None, ptr(rem)), "NULL")
        refused(fn(ctx, 77, ptr(c), v, count, ptr(pt), ptr(out), None), "curve")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt_r), ptr(out), None), "point[1] is not below r")
        refused(fn(ctx, C.curve_id, ptr(c), v, MAX_COUNT + 1, ptr(pt), ptr(out), None), "ARK355_POLY_MAX_COUNT")
        refused(fn(ctx, C.curve_id, None, 41, 1, None, None, None), "40")
        refused(fn(ctx, C.curve_id, None, 30, 1024, None, None, None), "2^40")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), ptr(c), None), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), ptr(out), vp(c.ctypes.data + 32)), "overlap")
        refused(fn(ctx, C.curve_id, ptr(c), v, count, ptr(pt), ptr(out), vp(out.ctypes.data + 32 * 15)), "overlap")
        refused(fn(None, C.curve_id, ptr(c), v, count, ptr(pt), ptr(out), None), message=False)
        assert fn(ctx, C.curve_id, None, v, 0, ptr(pt), None, None) == B.OK                  # count = 0: nothing to do
    # ---- open_dev: the handles
    O = BN254 if C is BLS12_381 else BLS12_381
    key = Key(lib, ctx, C, io, 1, [rnd.randrange(1, p) for _ in range(v)])
    g2_h = lib.bases_load(ctx, C.curve_id, 2, Z.g2_raw(C, C.g2_gen) * 4, 4)
    alien = lib.bases_load(ctx, O.curve_id, 1, Z.g1_raw(O, O.g1_gen) * 4, 4)
    try:
        proofs = np.zeros(3 * 512, dtype=np.uint8)
        value = np.zeros(32, dtype=np.uint8)
        arr = lambda hs: (vp * len(hs))(*hs)                   # noqa: E731
        L = key.levels
        opn = d.ark355_mle_open_dev
        refused(opn(ctx, C.curve_id, None, ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "level_bases is NULL")
        refused(opn(ctx, C.curve_id, arr([L[0], None, L[2]]), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "level 1 is NULL")
        refused(opn(ctx, C.curve_id, arr([L[0], L[1], alien]), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "level 2 belongs to another curve")
        refused(opn(ctx, C.curve_id, arr([L[0], g2_h, L[2]]), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "G1 and G2")
        refused(opn(ctx, C.curve_id, arr([L[0], L[2], L[2]]), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "level 1 holds 1 bases")
        refused(opn(ctx, C.curve_id, arr([L[1], L[1], L[2]]), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "level 0 holds 2 bases")
        refused(opn(ctx, C.curve_id, arr(L), None, v, ptr(pt), ptr(proofs), ptr(value)), "NULL")
        refused(opn(ctx, C.curve_id, arr(L), ptr(c), v, None, ptr(proofs), ptr(value)), "NULL")
        refused(opn(ctx, C.curve_id, arr(L), ptr(c), v, ptr(pt), None, ptr(value)), "NULL")
        refused(opn(ctx, C.curve_id, arr(L), ptr(c), v, ptr(pt), ptr(proofs), None), "NULL")
        refused(opn(ctx, 77, arr(L), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), "curve")
        refused(opn(ctx, C.curve_id, arr(L), ptr(c), v, ptr(pt_r), ptr(proofs), ptr(value)), "point[1] is not below r")
        refused(opn(ctx, C.curve_id, None, ptr(c), 41, None, None, ptr(value)), "40")
        refused(opn(ctx, C.curve_id, None, ptr(c), 40, None, None, ptr(value)), "2^40")
        refused(opn(None, C.curve_id, arr(L), ptr(c), v, ptr(pt), ptr(proofs), ptr(value)), message=False)
        assert not proofs.any() and not value.any(), "a refused open wrote"
        check_open(key, io, [rnd.randrange(p) for _ in range(1 << v)], point, (C.name, "after the refusals"))
    finally:
        key.free()
        d.ark355_bases_free(g2_h)
        d.ark355_bases_free(alien)


# ---- [GPU only] -------------------------------------------------------------------------------------------------------------------
def large_case(lib, ctx, C, io, policy, v=23, split=10, samples=64):
    """2^23 entries at E = 8 take a third pass (2048 x 2048 x 2).  Byte identity with the E = 2 run; the value against
    ark355_mle_eval_fr_dev; the levels from `split` on against the reference on ark355_mle_fix_fr_dev(k = split)'s 2^(v-split)
    entries; `samples` entries of each level below against a reference fold of the 2^(j+1) inputs that feed each"""
    p = C.r
    rnd = random.Random("mle-open/large/%d" % C.curve_id)
    N = 1 << v
    words = np.random.default_rng(0x0BE4 + C.curve_id).integers(0, 256, size=(N, 32), dtype=np.uint8)
    words[:, 31] &= (1 << ((p >> 248).bit_length() - 1)) - 1    # words below r: valid Montgomery images
    d_f, k_f = io.to_dev(words.tobytes())
    point = [rnd.randrange(p) for _ in range(v)]
    pb = point_bytes(point)
    d_q, k_q = io.alloc((N + 1) * 32)
    d_r, k_r = io.alloc(64)
    runs = {}
    for E in (2, 8):
        policy.setenv(POLICY, E)
        lib.mle_quotients_fr_dev(ctx, C.curve_id, d_f, v, 1, pb, d_q, d_r)
        runs[E] = io.read(k_q, (N + 1) * 32)
        assert runs[E][N * 32:] == A5 and io.read(k_r, 64)[32:] == A5
    policy.setenv(POLICY, E_DEFAULT)
    q = runs[8]
    assert q == runs[2], (C.name, "MLE_OPEN_LANE_ENTRIES = 8 against 2", qc.first_difference(q, runs[2]))
    d_e, k_e = io.alloc(64)
    lib.mle_eval_fr_dev(ctx, C.curve_id, d_f, v, 1, pb, d_e)
    assert io.read(k_e, 32) == q[(N - 1) * 32:N * 32] == io.read(k_r, 32), (C.name, "the value against mle_eval_fr_dev")
    M = N >> split
    d_g, k_g = io.alloc(M * 32)
    lib.mle_fix_fr_dev(ctx, C.curve_id, d_f, v, 1, point_bytes(point[:split]), split, d_g)
    levels, y = quot_ref(p, raw(io.read(k_g, M * 32)), point[split:])
    tail = unraw([x for lv in levels for x in lv] + [y])
    assert q[level(v, split)[0] * 32:N * 32] == tail, (C.name, "levels %d .. %d" % (split, v - 1))
    for j in range(split):
        off, ln = level(v, j)
        for i in [0, ln - 1] + [rnd.randrange(ln) for _ in range(samples - 2)]:
            src = [int.from_bytes(words[k].tobytes(), "little") for k in range(i << (j + 1), (i + 1) << (j + 1))]
            for r in point[:j]:
                src = fold_ref(p, src, r)
            assert raw(q[(off + i) * 32:(off + i + 1) * 32])[0] == (src[1] - src[0]) % p, (C.name, "level %d entry %d" % (j, i))
    assert io.read(k_f, 64) == words.tobytes()[:64]
