"""Every device field primitive against plain Python integers, at the operands where multi-limb arithmetic goes wrong -- shared by
the CPU-emulator tier (tests/test_emul_fieldops.py) and the GPU tier (tests/test_gpu_fieldops.py), through the test entry
ark355_diag_field_ops (one lane per element, the production functions on the production parameter classes).

The reference is Python integers only: nothing is imported from the library but the entry's wrapper and its code tables; the
oracle supplies p, r and the limb counts.  Layers and what they are compared with:

  Fp  (csrc/field.cuh, 32-bit limbs)   the 17 Montgomery-image patterns of field_edge_cases.montgomery_images and 4096 seeded
       operands, per field: unary ops on all of them, binary ops on all 289 ordered pairs, mul2sum / mul_sub on all 17^4 ordered
       quadruples; exact canonical integers, limb for limb.
  Fp2 the 289 elements whose components run over the images: all 289^2 ordered pairs, integer arithmetic in F_p[u]/(u^2 + 1).
  Fp28 (csrc/field28.cuh, radix 2^28, lazy limbs)   operands built as explicit limbs in the classes (a) .. (f) below; every operand
       is checked in Python against the documented precondition of the op it is sent to BEFORE the call (the emulator build aborts
       the process on a violated bound; the device build computes garbage), and every expected value is exact.

Readings taken where a comment of field28.cuh left room (each is asserted next to its use, and the comment was tightened to match):
  * sub<K, BETA> / neg<K, BETA>: the operand taken away must satisfy b.l[i] <= bias<K, BETA>(i) limb for limb -- limbs below the
    top one <= BETA (2^28 - 1) and the top limb <= (top limb of K p) - BETA.  "value < (K - 1) p" alone does not give the second
    on BN254, whose p has top limb 3: a normalised value just below 4 p has top limb 12, bias<5, 4> has 11.
  * products: besides the limb bounds (x + y <= 60 / 59 / 58 for one / two / four products, every limb < 2^31, sqr < 2^29.6) the
    operand VALUES must leave the result's top limb inside 32 bits: (sum a_j b_j) / R' + p < 2^(28 (N - 1) + 32).
  * "< 1.05 p whenever the product of the operand values is < 2^10 p^2" holds on BN254 only; the result is < p (1 + V / (p R')), so
    < 1.05 p needs V < 0.05 p R': V < 125 p^2 on BLS12-381 (R' / p = 2519).  The bound asserted here is the exact one.
  * norm / canon / to_fp / is_zero_mod_p: "any lazy value" means limbs whose carry chain stays inside 32 bits; limbs < 2^31 here.
  * cond_sub<K> "on operands that straddle K p": K p - 1, K p, K p + 1, K p -+ 2^(28 i) for every limb boundary i, and for every
    boundary the two values around "K p with the limbs below i cleared" (a borrow that runs through i limbs, and none).
"""
from __future__ import annotations

import ctypes as C
import itertools
import random
from fractions import Fraction

import numpy as np

from field_edge_cases import montgomery_images
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, FLD, FOP, FOP28

SEED = 0xF1E1D
N_RANDOM = 4096
TAIL_SIZES = (1, 255, 256, 257, 300)        # 300: not a multiple of the wave size (64)

# ---- the fields ---------------------------------------------------------------------------------------------------------------------
FP_FIELDS = {"BlsFq": (BLS12_381.q, BLS12_381.fq_bytes), "BlsFr": (BLS12_381.r, BLS12_381.fr_bytes),
             "BnFq": (BN254.q, BN254.fq_bytes), "BnFr": (BN254.r, BN254.fr_bytes)}
FP2_FIELDS = {"BlsFq2": "BlsFq", "BnFq2": "BnFq"}
FP28_FIELDS = {"BlsFq28": "BlsFq", "BnFq28": "BnFq"}

# every (K, BETA) with which csrc/msm28_impl.cuh and csrc/tails28_impl.cuh instantiate Fp28::sub / Fp28::neg, read from those files:
#   sub: <3,1> (add28, add28_g2, madd28z R, madd28_g2_head R, sqr<3>), <5,1> (sqr<5>), <6,1> (sqr<6>, sqr_x<6>), <8,1> (Pd of the
#        mixed additions, T = Q - X3, L::mul<8,1> has no sub), <11,1> (sqr_x<11>)
#   neg: <2,1> (py, both_of<2,1>, mul<2,1>), <3,1> (3p - Y1, mul<3,1>), <3,3> (both_of<3,3>), <4,2> (dbl28_g2_coord_ni),
#        <4,3> (both_of<4,3>, mul2<.,.,4,3>), <5,1> (mul2<5,1,..>), <5,4> (5p - W), <6,1> (both_with<6,1>, mul<6,1>, mul2<6,1,..>),
#        <8,1> (mul<8,1>)
SUB_CLASSES = ((3, 1), (5, 1), (6, 1), (8, 1), (11, 1))
NEG_CLASSES = ((2, 1), (3, 1), (3, 3), (4, 2), (4, 3), (5, 1), (5, 4), (6, 1), (8, 1))
COND_SUB_K = (1, 2, 4, 8, 16)

FP_OPS = ("add", "sub", "neg", "dbl", "mul", "mul_ni", "sqr", "mul2sum", "mul_sub", "inv", "to_mont", "from_mont")
FP2_OPS = ("add", "sub", "neg", "mul", "mul_ni", "sqr", "sqr_ni", "inv", "mul_sub")
FP28_OPS = (("from_fp", "to_fp", "to_fp_lt8", "norm", "canon", "is_zero_mod_p", "is_zero_mod_p_inl", "multiple_hint", "add", "mul", "sqr",
             "mul2sum", "mul4sum") + tuple("cond_sub<%d>" % k for k in COND_SUB_K)
            + tuple("sub<%d,%d>" % kb for kb in SUB_CLASSES) + tuple("neg<%d,%d>" % kb for kb in NEG_CLASSES))


def op_code(field, op):
    """The entry's code of op name `op` as field `field` would spell it"""
    if op.startswith("cond_sub<"):
        return FOP28["cond_sub"] + COND_SUB_K.index(int(op[9:-1]))
    if op.startswith(("sub<", "neg<")):
        k, b = (int(v) for v in op[4:-1].split(","))
        return FOP28[op[:3]] + 16 * k + b
    return FOP28[op] if field in FP28_FIELDS else FOP[op]


# (field, op) -> reason, for every combination that is NOT run: each is tested as a refusal (refusal_cases)
def _refusal_table():
    t = {}
    for f in FP_FIELDS:
        t[(f, "sqr_ni")] = "Fp has no out-of-line square of its own (sqr_ni is mul_ni(a, a)): not wired"
    for op in ("mul2sum", "mul_sub"):
        t[("BlsFr", op)] = "Fp::mul2sum needs two spare top bits (static assertion): r has 255 bits in 256"
    for f in FP2_FIELDS:
        for op in ("dbl", "mul2sum", "to_mont", "from_mont"):
            t[(f, op)] = "Fp2 has no such function the kernels call (dbl is add(a, a); no dual product; no Montgomery conversion)"
    return t


REFUSED = _refusal_table()
# the table of what runs: every (field, op) a *_case below must drive
TABLE = ([(f, op) for f in FP_FIELDS for op in FP_OPS if (f, op) not in REFUSED]
         + [(f, op) for f in FP2_FIELDS for op in FP2_OPS] + [(f, op) for f in FP28_FIELDS for op in FP28_OPS])
# raw codes no field accepts, and Fp28 bias classes no kernel instantiates
UNKNOWN_OPS = (13, 31, 45, 53, 0x100, 0x200, 0x100 + 16 * 2 + 1, 0x100 + 16 * 8 + 2, 0x200 + 16 * 11 + 1, 0x200 + 16 * 5 + 2, -1, 0x300)
UNKNOWN_FIELDS = (-1, 8, 99)


# ---- limbs <-> integers -------------------------------------------------------------------------------------------------------------
def to_words(vals, nwords):
    """non-negative integers -> (len, nwords) uint32, little-endian 32-bit limbs"""
    b = b"".join(v.to_bytes(4 * nwords, "little") for v in vals)
    return np.frombuffer(b, dtype="<u4").reshape(len(vals), nwords).astype(np.uint32)


class Mismatch(AssertionError):
    pass


def compare(field, op, got, expected, what="limbs"):
    """The comparer: `got` and `expected` are (n, words) uint32 arrays; a difference in any word fails, naming the field, the op and
    the index of the first operand tuple that differs."""
    got, expected = np.asarray(got, dtype=np.uint32), np.asarray(expected, dtype=np.uint32)
    assert got.shape == expected.shape, (field, op, got.shape, expected.shape)
    bad = np.nonzero((got != expected).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        raise Mismatch("%s.%s: %d of %d results differ; first at operand index %d: got %s %s, expected %s"
                       % (field, op, len(bad), got.shape[0], i, what, [hex(int(v)) for v in got[i]], [hex(int(v)) for v in expected[i]]))


class Runner:
    """Calls the entry, checks the flavour word and records every (field, op) it ran, in order."""

    def __init__(self, lib, ctx, flavour):
        self.lib, self.ctx, self.flavour, self.ran = lib, ctx, flavour, []

    def run(self, field, op, operands, out_words):
        n = operands[0].shape[0]
        assert all(o.shape[0] == n and o.dtype == np.uint32 for o in operands)
        res, fl = self.lib.diag_field_ops(self.ctx, FLD[field], op_code(field, op), operands, n, out_words)
        assert fl == self.flavour, "%s.%s: flavour word %d, this tier runs flavour %d" % (field, op, fl, self.flavour)
        self.ran.append((field, op))
        return res

    def check(self, field, op, operands, expected):
        compare(field, op, self.run(field, op, operands, expected.shape[1]), expected)


# ---- Fp -------------------------------------------------------------------------------------------------------------------------------
class FpRef:
    def __init__(self, name):
        self.name = name
        self.p, nbytes = FP_FIELDS[name]
        self.nw = nbytes // 4
        self.R = 1 << (8 * nbytes)
        self.Rinv = pow(self.R, -1, self.p)
        self.images = montgomery_images(self.p, nbytes)
        rng = random.Random(SEED ^ self.p)
        self.rand = [rng.randrange(self.p) for _ in range(N_RANDOM)]

    def words(self, vals):
        assert all(0 <= v < self.p for v in vals)
        return to_words(vals, self.nw)

    # the expected values: exact canonical integers
    def expect(self, op, *x):
        p, R, Ri = self.p, self.R, self.Rinv
        if op == "add":
            return (x[0] + x[1]) % p
        if op == "sub":
            return (x[0] - x[1]) % p
        if op == "neg":
            return -x[0] % p
        if op == "dbl":
            return 2 * x[0] % p
        if op in ("mul", "mul_ni"):
            return x[0] * x[1] * Ri % p
        if op == "sqr":
            return x[0] * x[0] * Ri % p
        if op == "mul2sum":
            return (x[0] * x[1] + x[2] * x[3]) * Ri % p
        if op == "mul_sub":
            return (x[0] * x[1] - x[2] * x[3]) * Ri % p
        if op == "inv":                      # a^(p-2) of the element whose image is x: 0 -> 0
            return pow(x[0] * Ri % p, p - 2, p) * R % p
        if op == "to_mont":
            return x[0] * R % p
        if op == "from_mont":
            return x[0] * Ri % p
        raise KeyError(op)


ARITY = {"add": 2, "sub": 2, "neg": 1, "dbl": 1, "mul": 2, "mul_ni": 2, "sqr": 1, "sqr_ni": 1, "mul2sum": 4, "mul_sub": 4, "inv": 1,
         "to_mont": 1, "from_mont": 1}


def fp_operand_tuples(F, arity, full_quads=True):
    """Index tuples into F.images + F.rand: all ordered tuples of the 17 images, then random tuples"""
    ni = len(F.images)
    pool = F.images + F.rand
    rng = random.Random(SEED + arity)
    if arity == 1:
        idx = [(i,) for i in range(len(pool))]
    elif arity == 2:
        idx = list(itertools.product(range(ni), repeat=2)) + [(ni + i, rng.randrange(len(pool))) for i in range(N_RANDOM)]
    else:
        if full_quads:
            idx = list(itertools.product(range(ni), repeat=4))
        else:       # the cross of the 289 pairs with the 17 diagonal pairs
            idx = [(a, b, c, c) for a in range(ni) for b in range(ni) for c in range(ni)]
        idx += [tuple(rng.randrange(len(pool)) for _ in range(4)) for _ in range(N_RANDOM)]
    return pool, np.array(idx, dtype=np.int64)


def fp_case(run, name, full_quads=True):
    """Every Fp op of the table on field `name`"""
    F = FpRef(name)
    cache = {}
    for op in FP_OPS:
        if (name, op) in REFUSED:
            continue
        arity = ARITY[op]
        key = (arity, full_quads)
        if key not in cache:
            pool, idx = fp_operand_tuples(F, arity, full_quads)
            cache[key] = (pool, idx, F.words(pool))
        pool, idx, pw = cache[key]
        operands = [pw[idx[:, j]] for j in range(arity)]
        expected = F.words([F.expect(op, *(pool[j] for j in t)) for t in idx.tolist()])
        if arity == 4:
            assert len(idx) >= (17 ** 4 if full_quads else 17 ** 3) + N_RANDOM
        run.check(name, op, operands, expected)


# ---- Fp2 ------------------------------------------------------------------------------------------------------------------------------
class Fp2Ref:
    def __init__(self, name):
        self.name = name
        self.B = FpRef(FP2_FIELDS[name])
        B = self.B
        self.elems = list(itertools.product(B.images, repeat=2))            # 289 elements (c0, c1)
        rng = random.Random(SEED ^ (B.p >> 7))
        self.rand = [(rng.randrange(B.p), rng.randrange(B.p)) for _ in range(N_RANDOM)]

    def words(self, elems):
        return np.concatenate([self.B.words([e[0] for e in elems]), self.B.words([e[1] for e in elems])], axis=1)

    def mont_mul(self, a, b):               # (a0 + a1 u)(b0 + b1 u) R^-1 in F_p[u]/(u^2 + 1)
        p, Ri = self.B.p, self.B.Rinv
        return ((a[0] * b[0] - a[1] * b[1]) * Ri % p, (a[0] * b[1] + a[1] * b[0]) * Ri % p)

    def expect(self, op, *x):
        p, R, Ri = self.B.p, self.B.R, self.B.Rinv
        if op == "add":
            return ((x[0][0] + x[1][0]) % p, (x[0][1] + x[1][1]) % p)
        if op == "sub":
            return ((x[0][0] - x[1][0]) % p, (x[0][1] - x[1][1]) % p)
        if op == "neg":
            return (-x[0][0] % p, -x[0][1] % p)
        if op in ("mul", "mul_ni"):
            return self.mont_mul(x[0], x[1])
        if op in ("sqr", "sqr_ni"):
            return self.mont_mul(x[0], x[0])
        if op == "mul_sub":
            u, v = self.mont_mul(x[0], x[1]), self.mont_mul(x[2], x[3])
            return ((u[0] - v[0]) % p, (u[1] - v[1]) % p)
        if op == "inv":                     # (a0 - a1 u) / (a0^2 + a1^2) of the element whose image is x; 0 -> 0
            a0, a1 = x[0][0] * Ri % p, x[0][1] * Ri % p
            ni = pow((a0 * a0 + a1 * a1) % p, p - 2, p)
            return (a0 * ni * R % p, -a1 * ni * R % p)
        raise KeyError(op)


def fp2_fixed_pairs(F2):
    """The fixed (c, d) pairs of mul_sub: zero, one, (p-1, p-1), (x, p - x), and Montgomery-image edges; at least 17"""
    p, B = F2.B.p, F2.B
    one = (B.R % p, 0)
    x = B.images[7]
    els = [(0, 0), one, (p - 1, p - 1), (x, p - x), (0, 1), (p - 1, 0), (0, p - 1), (1, 1), (B.R % p, B.R % p), ((p - 1) // 2, (p + 1) // 2),
           (B.images[10], B.images[11]), (B.images[13], B.images[14]), (B.images[15], B.images[16]), (p - 2, 1), ((1 << 32) - 1, 1 << 32)]
    pairs = [((0, 0), (0, 0)), (one, one), ((p - 1, p - 1), (p - 1, p - 1)), ((x, p - x), (x, p - x)), ((x, p - x), (p - x, x))]
    pairs += [(els[i], els[(i * 5 + 3) % len(els)]) for i in range(len(els))]
    assert len(pairs) >= 17
    return pairs


def fp2_case(run, name):
    F2 = Fp2Ref(name)
    E, ne = F2.elems, len(F2.elems)
    assert ne == 289
    rng = random.Random(SEED + 2)
    pool = E + F2.rand
    pw = F2.words(pool)
    pair_idx = list(itertools.product(range(ne), repeat=2)) + [(ne + i, rng.randrange(len(pool))) for i in range(N_RANDOM)]
    pair_idx = np.array(pair_idx, dtype=np.int64)
    assert len(pair_idx) == 289 * 289 + N_RANDOM
    una_idx = np.arange(len(pool), dtype=np.int64).reshape(-1, 1)
    shared = {}
    for op in FP2_OPS:
        if op == "mul_sub":
            fixed = fp2_fixed_pairs(F2)
            fw = (F2.words([c for c, d in fixed]), F2.words([d for c, d in fixed]))
            quads = [(a, b, k) for a in range(17 * 0, ne) for b in (a, (a * 7 + 1) % ne) for k in range(len(fixed))]
            # the cross of 289 (a, b) pairs -- element a with elements a and 7a + 1 -- with the fixed list, and random quadruples
            qa = np.array([q[0] for q in quads]); qb = np.array([q[1] for q in quads]); qk = np.array([q[2] for q in quads])
            operands = [pw[qa], pw[qb], fw[0][qk], fw[1][qk]]
            exp = [F2.expect(op, pool[a], pool[b], fixed[k][0], fixed[k][1]) for a, b, k in quads]
            ridx = [tuple(rng.randrange(len(pool)) for _ in range(4)) for _ in range(N_RANDOM)]
            operands = [np.concatenate([o, pw[np.array([t[j] for t in ridx])]]) for j, o in enumerate(operands)]
            exp += [F2.expect(op, *(pool[j] for j in t)) for t in ridx]
            run.check(name, op, operands, F2.words(exp))
            continue
        arity = ARITY[op]
        idx = pair_idx if arity == 2 else una_idx
        ref_op = {"mul_ni": "mul", "sqr_ni": "sqr"}.get(op, op)
        if ref_op not in shared:
            shared[ref_op] = F2.words([F2.expect(ref_op, *(pool[j] for j in t)) for t in idx.tolist()])
        run.check(name, op, [pw[idx[:, j]] for j in range(arity)], shared[ref_op])


# ---- Fp28 -----------------------------------------------------------------------------------------------------------------------------
class Fp28Ref:
    """The representation of csrc/field28.cuh restated in integers: N limbs of 28 bits, value = sum l[i] 2^(28 i)."""

    def __init__(self, name):
        self.name = name
        self.B = FpRef(FP28_FIELDS[name])
        p = self.p = self.B.p
        self.NB = self.B.nw
        self.N = (p.bit_length() + 8 + 27) // 28
        self.RB = 28 * self.N
        self.SHIFT = self.RB - 32 * self.NB
        assert 0 <= self.SHIFT < 32 and (self.N, self.NB) in ((14, 12), (10, 8))
        self.Rp = 1 << self.RB
        self.MASK = (1 << 28) - 1
        self.pinv_Rp = pow(p, -1, self.Rp)
        self.top_shift = 28 * (self.N - 1)

    def norm(self, v):
        """the normalised limbs of integer v: 28 bits each, the top limb keeps what is left (must fit 32 bits)"""
        assert 0 <= v < 1 << (self.top_shift + 32)
        return [(v >> (28 * i)) & self.MASK for i in range(self.N - 1)] + [v >> self.top_shift]

    def val(self, limbs):
        return sum(int(l) << (28 * i) for i, l in enumerate(limbs))

    def bias(self, k, beta):
        """make_bias: k p with every limb but the top one raised by beta 2^28, the borrow taken from the next limb"""
        d = self.norm(k * self.p)
        for i in range(self.N):
            if i == 0:
                d[i] += beta << 28
            elif i == self.N - 1:
                d[i] -= beta
            else:
                d[i] += (beta << 28) - beta
        assert d[-1] >= 0 and self.val(d) == k * self.p and all(0 <= x < 1 << 32 for x in d)
        return d

    def limb_sum(self, *ls):
        s = [sum(t) for t in zip(*ls)]
        assert all(x < 1 << 32 for x in s)
        return s

    def arr(self, list_of_limbs):
        a = np.array(list_of_limbs, dtype=np.uint64)
        assert a.ndim == 2 and a.shape[1] == self.N and (a < (1 << 32)).all()
        return a.astype(np.uint32)

    def from_fp(self, x):
        return (x << self.SHIFT) % self.p

    def to_fp(self, v):
        return (v % self.p) * pow(1 << self.SHIFT, -1, self.p) % self.p

    def product(self, pairs):
        """(sum a_j b_j + m p) / R' with m = -(sum a_j b_j) p^-1 mod R': the exact integer the product pass returns"""
        s = sum(a * b for a, b in pairs)
        m = -s * self.pinv_Rp % self.Rp
        q, rem = divmod(s + m * self.p, self.Rp)
        assert rem == 0
        return q

    # ---- operand classes (explicit limbs) ----
    def class_a(self):
        return [self.norm(self.from_fp(x)) for x in self.B.images]

    def forms_of(self, k, delta):
        """k p + delta (delta in -1, 0, 1) as limbs: normalised, a limb-wise sum of two and of three normalised values, and the
        borrow-friendly form of make_bias with the delta added to limb 0"""
        p, v = self.p, k * self.p + delta
        if v < 0:
            return []
        out = [self.norm(v)]
        j = k // 2
        if k - j >= 1 or delta >= 0:
            a, b = j * p, (k - j) * p + delta
            if b >= 0:
                out.append(self.limb_sum(self.norm(a), self.norm(b)))
        if k >= 3:
            out.append(self.limb_sum(self.norm(p), self.norm((k - 2) * p + delta), self.norm(p)))
        for beta in (1, 3):
            if k >= 1 and self.norm(k * p)[-1] >= beta:
                d = self.bias(k, beta)
                d[0] += delta
                out.append(d)
        assert all(self.val(o) == v for o in out) and len(out) >= (3 if k >= 1 else 1)
        return out

    def class_d(self):
        A = self.class_a()
        rng = random.Random(SEED + 4)
        out = []
        for m in (2, 3, 4):
            out += [self.limb_sum(*(A[(i + j * (m + 1)) % len(A)] for j in range(m))) for i in range(len(A))]
            out += [self.limb_sum(*(rng.choice(A) for _ in range(m))) for _ in range(17)]
        return out

    def wide(self, bound, pattern, top_cap=None):
        """class (e): limbs at the bound of a product pass: `pattern` in all / low / high / even / odd selects which limbs are
        bound - 1 (the others are zero), as run_kara of tests/cpp/test_madd28_emul.cpp does.  The top limb is capped so that the
        VALUE stays below 2^11 p (the N class of the header): a value bound, not a limb bound, keeps the result inside N limbs."""
        N, H = self.N, self.N // 2
        cap = ((self.p << 11) >> self.top_shift) if top_cap is None else top_cap
        sel = {"all": lambda i: True, "low": lambda i: i < H, "high": lambda i: i >= H, "even": lambda i: i % 2 == 0,
               "odd": lambda i: i % 2 == 1}[pattern]
        l = [(bound - 1) if sel(i) else 0 for i in range(N)]
        l[-1] = min(l[-1], cap)
        return l

    def class_f(self, count, kmax=8, lazy=False):
        """random N-form values below kmax p (lazy: limb-wise sums of two or three of them)"""
        rng = random.Random(SEED + 6 + kmax + (100 if lazy else 0))
        if not lazy:
            return [self.norm(rng.randrange(kmax * self.p)) for _ in range(count)]
        return [self.limb_sum(*(self.norm(rng.randrange(kmax * self.p // 3)) for _ in range(rng.choice((2, 3))))) for _ in range(count)]


PATTERNS = ("all", "low", "high", "even", "odd")


def _product_precondition(F, xs, ys, what):
    """The documented contract of mul / mul2sum / mul4sum (header of field28.cuh and `mulsum_school`): with J = len(xs) products of
    limb bounds 2^x_j, 2^y_j, the column N sum_j 2^(x_j + y_j) + N 2^56 + 2^37 stays below 2^64 (J = 1: x + y <= 60, J = 2: 59,
    J = 4: 58); every limb is below 2^31 (the Karatsuba level); the result's top limb fits 32 bits (value reading, see the module
    docstring)."""
    n = xs[0].shape[0]
    col = np.zeros(n, dtype=object)
    for x, y in zip(xs, ys):
        assert (x < (1 << 31)).all() and (y < (1 << 31)).all(), what
        mx = [int(v) for v in x.max(axis=1)]
        my = [int(v) for v in y.max(axis=1)]
        col = col + np.array([F.N * a * b for a, b in zip(mx, my)], dtype=object)
    assert all(int(c) + F.N * (1 << 56) + (1 << 37) < 1 << 64 for c in col), what


def _column_bound_ok(F, t):
    """the column bound of _product_precondition for one tuple (x0, y0, x1, y1, ..) of limb lists"""
    return F.N * sum(max(t[j]) * max(t[j + 1]) for j in range(0, len(t), 2)) + F.N * (1 << 56) + (1 << 37) < 1 << 64


def _admissible(F, tuples, n_designed):
    """Tuples mixed from the general pools are kept only where they satisfy the column bound of their pass (lazy forms at 2^30
    against each other do not fit a dual product); the last n_designed tuples were built AT the bound and must all satisfy it."""
    assert all(_column_bound_ok(F, t) for t in tuples[-n_designed:])
    kept = [t for t in tuples if _column_bound_ok(F, t)]
    assert len(kept) >= n_designed + 100
    return kept


def _products_expected(F, xs, ys):
    n = xs[0].shape[0]
    vx = [[F.val(r) for r in x.tolist()] for x in xs]
    vy = [[F.val(r) for r in y.tolist()] for y in ys]
    out = []
    for i in range(n):
        pairs = [(vx[j][i], vy[j][i]) for j in range(len(xs))]
        q = F.product(pairs)
        assert q < 1 << (F.top_shift + 32), "operand values too large for the result's top limb"
        V = sum(a * b for a, b in pairs)
        # the header's value bound, exact form: result < p (1 + V / (p R')); < 1.05 p whenever V < 0.05 p R'
        assert q * F.Rp < V + F.p * F.Rp + F.Rp
        if 20 * V < F.p * F.Rp:
            assert 100 * q < 105 * F.p
        if F.name == "BnFq28" and V < (F.p * F.p) << 10:          # the header's own wording holds where R' / p >= 2^14.4
            assert 100 * q < 105 * F.p
        out.append(F.norm(q))
    return F.arr(out)


def fp28_case(run, name):
    """Every Fp28 op of the table on field `name`"""
    F = Fp28Ref(name)
    p, N = F.p, F.N
    A = F.class_a()
    Bforms = [(k, f) for k in range(32) for f in F.forms_of(k, 0)]                                   # class (b)
    Cforms = [(k, d, f) for k in range(32) for d in (1, -1) for f in F.forms_of(k, d)]              # class (c)
    D = F.class_d()
    assert len({k for k, f in Bforms}) == 32 and sum(1 for k, f in Bforms if k == 9) >= 3
    lt32 = A + [f for k, f in Bforms] + [f for k, d, f in Cforms] + D + F.class_f(256, 8) + F.class_f(256, 32) + F.class_f(256, 8, lazy=True)
    assert all(F.val(l) < 32 * p and max(l) < 1 << 31 for l in lt32)              # the input class of canon / to_fp / is_zero_mod_p
    lt32a = F.arr(lt32)
    vals32 = [F.val(l) for l in lt32]

    # from_fp, and to_fp(from_fp(x)) == x
    xs = F.B.images + F.B.rand[:512]
    xw = F.B.words(xs)
    got = run.run(name, "from_fp", [xw], N)
    compare(name, "from_fp", got, F.arr([F.norm(F.from_fp(x)) for x in xs]))
    compare(name, "to_fp", run.run(name, "to_fp", [got], F.NB), xw, what="to_fp(from_fp(x))")

    # canon / to_fp / the predicates on every lazy value < 32 p; to_fp_lt8 on those < 8 p
    run.check(name, "canon", [lt32a], F.arr([F.norm(v % p) for v in vals32]))
    run.check(name, "to_fp", [lt32a], F.B.words([F.to_fp(v) for v in vals32]))
    lt8 = [i for i, v in enumerate(vals32) if v < 8 * p]
    assert len(lt8) > 300
    run.check(name, "to_fp_lt8", [lt32a[lt8]], F.B.words([F.to_fp(vals32[i]) for i in lt8]))
    zero = [1 if v % p == 0 else 0 for v in vals32]
    nb, nc = len(A), len(Bforms)
    # true on every form of class (b); elsewhere only where the integer says so (the image 0, and the sums of class (d) whose
    # summands cancel: 1 and p - 1, (p - 1) / 2 and (p + 1) / 2 -- lazy forms of p the tables above do not build)
    assert all(zero[nb:nb + nc]) and zero[0] == 1 and nc < sum(zero) < nc + 40
    assert not any(zero[nb + nc:nb + nc + len(Cforms)])
    for op in ("is_zero_mod_p", "is_zero_mod_p_inl"):
        run.check(name, op, [lt32a], np.array(zero, dtype=np.uint32).reshape(-1, 1))

    # multiple_hint: k on every form of k p; elsewhere v p^-1 mod 2^28
    pinv28 = pow(p, -1, 1 << 28)
    hint = [v * pinv28 % (1 << 28) for v in vals32]
    assert all(hint[nb + i] == k for i, (k, f) in enumerate(Bforms))
    assert all(hint[nb + nc + i] >= 10 for i in range(len(Cforms))), "no neighbour of a multiple passes the `< 10` filter by its hint"
    run.check(name, "multiple_hint", [lt32a], np.array(hint, dtype=np.uint32).reshape(-1, 1))

    # norm: any lazy limbs whose carry chain stays inside 32 bits (limbs < 2^31 here)
    wide31 = [F.wide(1 << 31, pt) for pt in PATTERNS] + [F.wide(1 << 30, pt) for pt in PATTERNS]
    nin = lt32 + wide31
    run.check(name, "norm", [F.arr(nin)], F.arr([F.norm(F.val(l)) for l in nin]))

    # cond_sub<K> on normalised operands that straddle K p
    for K in COND_SUB_K:
        kp = K * p
        cands = {kp - 1, kp, kp + 1, 0, 1, 2 * kp - 1, 2 * kp, kp // 2}
        for i in range(N):
            cands |= {kp - (1 << (28 * i)), kp + (1 << (28 * i))}
            cleared = (kp >> (28 * i)) << (28 * i)
            cands |= {cleared - 1, cleared, cleared + 1}
        cands |= {F.val(a) for a in A} | {F.val(l) for l in F.class_f(128, 2 * K)}
        cands = sorted(v for v in cands if 0 <= v and (v >> F.top_shift) < 1 << 31)
        run.check(name, "cond_sub<%d>" % K, [F.arr([F.norm(v) for v in cands])], F.arr([F.norm(v - kp if v >= kp else v) for v in cands]))

    # add: limb-wise
    L1 = A + D + F.class_f(128, 8, lazy=True) + wide31[5:]
    rng = random.Random(SEED + 28)
    pa = [(L1[i], L1[(3 * i + 1) % len(L1)]) for i in range(len(L1))] + [(rng.choice(L1), rng.choice(L1)) for _ in range(256)]
    assert all(x + y < 1 << 32 for a, b in pa for x, y in zip(a, b))
    run.check(name, "add", [F.arr([a for a, b in pa]), F.arr([b for a, b in pa])], F.arr([[x + y for x, y in zip(a, b)] for a, b in pa]))

    # sub<K, BETA> / neg<K, BETA>: the limb-wise integers of the definitions; value a - b + K p / K p - b
    norm_pool = A + F.class_f(64, 2) + [F.norm(k * p + d) for k in range(0, 11) for d in (-1, 0, 1) if k * p + d >= 0]
    for kind, classes in (("sub", SUB_CLASSES), ("neg", NEG_CLASSES)):
        for K, BETA in classes:
            bias = F.bias(K, BETA)
            top_ok = bias[-1]
            full = [BETA * F.MASK] * (N - 1) + [top_ok]                    # the widest operand of the class
            bs = [l for l in norm_pool + D + [F.limb_sum(*[a] * BETA) for a in A[:8]] if all(x <= c for x, c in zip(l, full))]
            bs += [full, list(bias[:-1]) + [top_ok], [0] * N, [BETA * F.MASK] * (N - 1) + [0], [0] * (N - 1) + [top_ok]]
            bs[-4] = [min(x, c) for x, c in zip(bias, full)]
            # precondition (reading in the module docstring): limb for limb below the bias
            assert len(bs) > 20 and all(x <= c and x <= BETA * F.MASK or i == N - 1 and x <= c for l in bs for i, (x, c) in enumerate(zip(l, bias)))
            if kind == "neg":
                exp = [[c - x for x, c in zip(l, bias)] for l in bs]
                assert all(F.val(e) == K * p - F.val(l) for e, l in zip(exp, bs))
                run.check(name, "neg<%d,%d>" % (K, BETA), [F.arr(bs)], F.arr(exp))
            else:
                As = [L1[(5 * i + K) % len(L1)] for i in range(len(bs))]
                assert all(a + c - x < 1 << 32 for l, al in zip(bs, As) for a, x, c in zip(al, l, bias))
                exp = [[a + c - x for a, x, c in zip(al, l, bias)] for l, al in zip(bs, As)]
                assert all(F.val(e) == F.val(al) - F.val(l) + K * p for e, al, l in zip(exp, As, bs))
                run.check(name, "sub<%d,%d>" % (K, BETA), [F.arr(As), F.arr(bs)], F.arr(exp))

    # ---- products ----
    kp_forms = [f for k, f in Bforms if k in (0, 1, 2, 9, 31)] + [f for k, d, f in Cforms if k in (1, 9, 31)]
    rnd = F.class_f(128, 8) + F.class_f(128, 6, lazy=True)

    def widths(bx, by):
        return [(F.wide(bx, pa_), F.wide(by, pb_)) for pa_ in PATTERNS for pb_ in PATTERNS]

    # mul: all ordered pairs of class (a); multiples of p and their neighbours; L1 x L1; the widest classes x + y = 60 with every limb < 2^31
    mp = list(itertools.product(A, A)) + [(a, b) for a in kp_forms for b in (A[2], A[7], kp_forms[-1])]
    mp += [(D[i], D[(7 * i + 3) % len(D)]) for i in range(len(D))] + [(rnd[i], rnd[-1 - i]) for i in range(len(rnd))]
    mp += widths(1 << 30, 1 << 30) + widths(1 << 31, 1 << 29) + widths(1 << 29, 1 << 31) + widths(1 << 28, 1 << 31)
    x, y = F.arr([a for a, b in mp]), F.arr([b for a, b in mp])
    _product_precondition(F, [x], [y], "mul")
    run.check(name, "mul", [x, y], _products_expected(F, [x], [y]))

    # sqr: limbs < 2^29.6; sqr(a) == mul(a, a) limb for limb
    b296 = int(2 ** 29.6)
    sq = A + kp_forms + D + rnd + [F.wide(b296, pt) for pt in PATTERNS] + [F.wide(1 << 29, pt) for pt in PATTERNS]
    sq = [l for l in sq if max(l) < b296]
    assert len(sq) > 200
    x = F.arr(sq)
    _product_precondition(F, [x], [x], "sqr")
    exp = _products_expected(F, [x], [x])
    got = run.run(name, "sqr", [x], N)
    compare(name, "sqr", got, exp)
    compare(name, "sqr", got, run.run(name, "mul", [x, x], N), what="sqr(a) against mul(a, a)")

    # mul2sum: x + y <= 59 for both products, or 59.6 + 57
    base = A + D[:34] + rnd[:64] + kp_forms
    q = [(base[i], base[(3 * i + 1) % len(base)], base[(5 * i + 2) % len(base)], base[(7 * i + 3) % len(base)]) for i in range(len(base))]
    q += [(a, b, A[2], A[2]) for a in A for b in A[:6]]
    b298, b285 = int(2 ** 29.8), int(2 ** 28.5)
    for pa_, pb_ in itertools.product(PATTERNS, PATTERNS):
        q.append((F.wide(1 << 30, pa_), F.wide(1 << 29, pb_), F.wide(1 << 29, pb_), F.wide(1 << 30, pa_)))
        q.append((F.wide(1 << 31, pa_), F.wide(1 << 28, pb_), F.wide(1 << 28, pa_), F.wide(1 << 31, pb_)))
        q.append((F.wide(b298, pa_), F.wide(b298, pb_), F.wide(b285, pb_), F.wide(b285, pa_)))
    q = _admissible(F, q, n_designed=3 * len(PATTERNS) ** 2)
    ops = [F.arr([t[j] for t in q]) for j in range(4)]
    _product_precondition(F, [ops[0], ops[2]], [ops[1], ops[3]], "mul2sum")
    run.check(name, "mul2sum", ops, _products_expected(F, [ops[0], ops[2]], [ops[1], ops[3]]))

    # mul4sum: x + y <= 58 for the four products
    q = [tuple(base[((2 * j + 3) * i + j) % len(base)] for j in range(8)) for i in range(len(base))]
    for pa_, pb_ in itertools.product(PATTERNS, PATTERNS):
        q.append((F.wide(1 << 29, pa_), F.wide(1 << 29, pb_)) * 4)
        q.append((F.wide(1 << 30, pa_), F.wide(1 << 28, pb_), F.wide(1 << 28, pa_), F.wide(1 << 30, pb_)) * 2)
        q.append((F.wide(1 << 31, pa_), F.wide(1 << 27, pb_), F.wide(1 << 27, pa_), F.wide(1 << 31, pb_)) * 2)
    q = _admissible(F, q, n_designed=3 * len(PATTERNS) ** 2)
    ops = [F.arr([t[j] for t in q]) for j in range(8)]
    _product_precondition(F, ops[0::2], ops[1::2], "mul4sum")
    run.check(name, "mul4sum", ops, _products_expected(F, ops[0::2], ops[1::2]))


# ---- the filter and its use -------------------------------------------------------------------------------------------------------------
# Every site that computes Pd = U2 - X1 + K p and then asks `Pd.multiple_hint() < 10`: (site, K, BETA, bound of U2 / p, bound of the
# accumulator coordinate / p), the bounds as the comments above those kernels state them.
PD_SITES = (("madd28z (msm28_impl.cuh)", 8, 1, Fraction(105, 100), Fraction(61, 10)),
            ("madd28_g2_head (msm28_impl.cuh)", 8, 1, Fraction(105, 100), Fraction(61, 10)),
            ("add28 (tails28_impl.cuh)", 3, 1, Fraction(105, 100), Fraction(105, 100)),
            ("add28_g2 (tails28_impl.cuh)", 3, 1, Fraction(105, 100), Fraction(105, 100)))
HINT_BOUND = 10


def pd_multiple_range(K, u2_bound, x1_bound):
    """U2 in [0, u2_bound p), X1 in [0, x1_bound p): Pd = U2 - X1 + K p lies in ((K - x1_bound) p, (K + u2_bound) p); the multiples
    k p inside that open interval"""
    lo, hi = K - x1_bound, K + u2_bound
    kmin = int(lo // 1) + 1
    kmax = int(-(-hi // 1)) - 1
    return kmin, kmax


def pd_filter_case():
    for site, K, BETA, u2, x1 in PD_SITES:
        assert (K, BETA) in SUB_CLASSES, site
        kmin, kmax = pd_multiple_range(K, u2, x1)
        assert 0 <= kmin <= kmax < HINT_BOUND, (site, kmin, kmax)
        assert x1 <= K - 1, site              # the coordinate taken away stays below (K - 1) p: Pd is positive
    assert pd_multiple_range(8, Fraction(105, 100), Fraction(61, 10)) == (2, 9)
    assert pd_multiple_range(3, Fraction(105, 100), Fraction(105, 100)) == (2, 4)
    assert pd_multiple_range(11, Fraction(105, 100), Fraction(61, 10))[1] >= HINT_BOUND        # a wider bias class trips it


# ---- tails, refusals, the comparer ----------------------------------------------------------------------------------------------------
TAIL_OPS = {"BlsFq": "mul", "BlsFr": "mul", "BnFq": "mul2sum", "BnFr": "sub", "BlsFq2": "mul", "BnFq2": "sqr", "BlsFq28": "mul", "BnFq28": "mul2sum"}


def tail_case(run, name):
    """One op of field `name` at n = 1, 255, 256, 257 and one n that is no multiple of the wave size, same expected values"""
    op = TAIL_OPS[name]
    nmax = max(TAIL_SIZES)
    if name in FP_FIELDS:
        F = FpRef(name)
        pool = (F.images * 20)[:nmax]
        arity = ARITY[op]
        tup = [tuple(pool[(i * (j + 1) + 3 * j) % nmax] for j in range(arity)) for i in range(nmax)]
        operands = [F.words([t[j] for t in tup]) for j in range(arity)]
        expected = F.words([F.expect(op, *t) for t in tup])
    elif name in FP2_FIELDS:
        F2 = Fp2Ref(name)
        pool = (F2.elems * 2)[:nmax]
        arity = ARITY[op]
        tup = [tuple(pool[(i * (j + 1) + 5 * j) % nmax] for j in range(arity)) for i in range(nmax)]
        operands = [F2.words([t[j] for t in tup]) for j in range(arity)]
        expected = F2.words([F2.expect(op, *t) for t in tup])
    else:
        F = Fp28Ref(name)
        pool = (F.class_a() + F.class_d())
        pool = (pool * (nmax // len(pool) + 1))[:nmax]
        arity = 2 if op == "mul" else 4
        operands = [F.arr([pool[(i * (j + 1) + 7 * j) % nmax] for i in range(nmax)]) for j in range(arity)]
        _product_precondition(F, operands[0::2], operands[1::2], op)
        expected = _products_expected(F, operands[0::2], operands[1::2])
    for n in TAIL_SIZES:
        got = run.run(name, op, [o[:n] for o in operands], expected.shape[1])
        assert got.shape[0] == n
        compare(name, op, got, expected[:n])


def table_is_complete():
    """Every (field, op name) is either run or refused with a reason; names of another field type are refused by their codes"""
    n_run = n_ref = 0
    for f in list(FP_FIELDS) + list(FP2_FIELDS) + list(FP28_FIELDS):
        own = FP_OPS if f in FP_FIELDS else FP2_OPS if f in FP2_FIELDS else FP28_OPS
        for op in (set(FP_OPS) | set(FP2_OPS)) if f not in FP28_FIELDS else FP28_OPS:
            assert ((f, op) in TABLE) != ((f, op) in REFUSED), (f, op)
            n_run += (f, op) in TABLE
            n_ref += (f, op) in REFUSED
        assert all((f, op) in TABLE or (f, op) in REFUSED for op in own)
    assert n_run == len(TABLE) == 46 + 18 + 64 and n_ref == len(REFUSED) == 4 + 2 + 8
    return n_run


def _raw_call(lib, ctx, field, code, operands, n, res, cap, fl):
    ptrs = (C.c_void_p * 8)(*[(o.ctypes.data if o is not None else None) for o in operands] + [None] * (8 - len(operands)))
    return lib.dll.ark355_diag_field_ops(ctx, field, code, ptrs, len(operands), n, res.ctypes.data if res is not None else None, cap,
                                         C.byref(fl) if fl is not None else None)


def refusal_cases(run):
    """Every uninstantiable combination of the table, ops of another field type, unknown ops and fields, NULL pointers, a wrong
    operand count, a short result buffer: ARK355_EINVAL each, nothing written, and the context works afterwards"""
    lib, ctx = run.lib, run.ctx
    a = np.zeros((4, 28), dtype=np.uint32)
    res = np.full((4, 28), 7, dtype=np.uint32)
    fl = C.c_uint32(7)

    def refused(field, code, operands=(a,) * 8, n=4, r=res, cap=4 * 28, f=fl, count=None):
        ops = list(operands) if count is None else list(operands)[:count]
        assert _raw_call(lib, ctx, field, code, ops, n, r, cap, f) == EINVAL, (field, code, len(ops))
        assert (res == 7).all() and fl.value == 7

    for (f, op), reason in REFUSED.items():
        assert reason
        code = op_code(f, op)
        for count in (1, 2, 4, 8):
            refused(FLD[f], code, count=count)
    for f in FLD:                                       # codes of another field type, unknown codes, unused bias classes
        own = {op_code(f, op) for ff, op in TABLE if ff == f}
        other = {op_code(ff, op) for ff, op in TABLE} - own
        for code in sorted(other) + list(UNKNOWN_OPS):
            if code in own:
                continue
            for count in (1, 2, 4, 8):
                refused(FLD[f], code, count=count)
    for field in UNKNOWN_FIELDS:
        refused(field, FOP["add"], count=2)
    # NULL pointers, a wrong operand count, capacity, n above the limit
    add = (FLD["BnFq"], FOP["add"])
    assert lib.dll.ark355_diag_field_ops(ctx, add[0], add[1], None, 2, 4, res.ctypes.data, 32, C.byref(fl)) == EINVAL
    refused(*add, operands=(a, None))
    refused(*add, operands=(None, a))
    assert _raw_call(lib, ctx, add[0], add[1], [a, a], 4, None, 32, fl) == EINVAL
    assert _raw_call(lib, ctx, add[0], add[1], [a, a], 4, res, 32, None) == EINVAL
    assert _raw_call(lib, None, add[0], add[1], [a, a], 4, res, 32, fl) == EINVAL
    for count in (0, 1, 3, 4, 8):
        refused(*add, count=count)
    refused(*add, count=2, cap=31)
    refused(*add, count=2, n=(1 << 24) + 1, cap=1 << 40)
    assert (res == 7).all() and fl.value == 7
    # the context still works
    F = FpRef("BnFq")
    x, y = F.images[:4], F.images[4:8]
    run.check("BnFq", "add", [F.words(x), F.words(y)], F.words([F.expect("add", u, v) for u, v in zip(x, y)]))


def comparer_bites():
    """A correct result array with ONE bit flipped in one limb of one element fails the comparer, which names the field, the op and
    the operand index -- for an Fp, an Fp2 and an Fp28 limb result and for a predicate word"""
    F, F2, F28 = FpRef("BlsFq"), Fp2Ref("BnFq2"), Fp28Ref("BlsFq28")
    good = {
        ("BlsFq", "mul"): F.words([F.expect("mul", a, b) for a, b in itertools.product(F.images, repeat=2)]),
        ("BnFq2", "sqr"): F2.words([F2.expect("sqr", e) for e in F2.elems]),
        ("BlsFq28", "canon"): F28.arr([F28.norm(F28.val(l) % F28.p) for l in F28.class_d()]),
        ("BlsFq28", "is_zero_mod_p"): np.array([[1 if k % 3 == 0 else 0] for k in range(96)], dtype=np.uint32),
    }
    for (field, op), exp in good.items():
        compare(field, op, exp.copy(), exp)
        n, w = exp.shape
        for idx, word, bit in ((0, 0, 0), (n - 1, w - 1, 31 if w > 1 else 0), (n // 2, w // 2, 13 if w > 1 else 0)):
            bad = exp.copy()
            bad[idx, word] ^= np.uint32(1 << bit)
            try:
                compare(field, op, bad, exp)
            except Mismatch as e:
                msg = str(e)
                assert msg.startswith("%s.%s:" % (field, op)) and ("operand index %d:" % idx) in msg and "1 of %d" % n in msg, msg
            else:
                raise AssertionError("the comparer accepted a flipped bit: %s.%s element %d word %d bit %d" % (field, op, idx, word, bit))
