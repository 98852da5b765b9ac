"""ark-serialize compatible encodings (oracle; restates the un-vendored ``ark-serialize`` +
``ark-bls12-381/src/curves/util.rs`` + ``ark-ec`` SW flags; SURVEY.md Appendix A "Serialisation").

* field elements: canonical (non-Montgomery) little-endian bytes;
* BLS12-381 points: zcash/IETF format -- big-endian x (G2: x.c1 || x.c0); top byte flags
  bit7 = compressed, bit6 = infinity, bit5 = y lexicographically largest;
* BN254 points: little-endian x (G2: c0 || c1), flags in the two top bits of the LAST byte:
  bit7 = y is "negative" (y > -y), bit6 = infinity;
* ``Vec<T>`` = u64 LE length then the elements; ``Proof`` = a || b || c.
"""
from __future__ import annotations

from .curves import g1 as _g1, g2 as _g2
from .fields import CurveParams


def _fq_gt_neg(y, q):
    return y > (q - y) % q


def _fq2_gt_neg(y, q):
    """Fq2 ordering: compare c1 first, then c0 (ark-ff QuadExtField Ord)."""
    n = ((-y[0]) % q, (-y[1]) % q)
    if y[1] != n[1]:
        return y[1] > n[1]
    return y[0] > n[0]


def g1_compressed(curve: CurveParams, P) -> bytes:
    q, nb = curve.q, curve.fq_bytes
    if curve.bn_like:
        if P is None:
            b = bytearray(nb)
            b[-1] |= 1 << 6
            return bytes(b)
        b = bytearray(P[0].to_bytes(nb, "little"))
        if _fq_gt_neg(P[1], q):
            b[-1] |= 1 << 7
        return bytes(b)
    if P is None:
        b = bytearray(nb)
        b[0] |= 0xC0
        return bytes(b)
    b = bytearray(P[0].to_bytes(nb, "big"))
    b[0] |= 0x80
    if _fq_gt_neg(P[1], q):
        b[0] |= 0x20
    return bytes(b)


def g2_compressed(curve: CurveParams, P) -> bytes:
    q, nb = curve.q, curve.fq_bytes
    if curve.bn_like:
        if P is None:
            b = bytearray(2 * nb)
            b[-1] |= 1 << 6
            return bytes(b)
        b = bytearray(P[0][0].to_bytes(nb, "little") + P[0][1].to_bytes(nb, "little"))
        if _fq2_gt_neg(P[1], q):
            b[-1] |= 1 << 7
        return bytes(b)
    if P is None:
        b = bytearray(2 * nb)
        b[0] |= 0xC0
        return bytes(b)
    b = bytearray(P[0][1].to_bytes(nb, "big") + P[0][0].to_bytes(nb, "big"))
    b[0] |= 0x80
    if _fq2_gt_neg(P[1], q):
        b[0] |= 0x20
    return bytes(b)


def g1_uncompressed(curve: CurveParams, P) -> bytes:
    q, nb = curve.q, curve.fq_bytes
    if curve.bn_like:
        if P is None:
            b = bytearray(2 * nb)
            b[-1] |= 1 << 6
            return bytes(b)
        b = bytearray(P[0].to_bytes(nb, "little") + P[1].to_bytes(nb, "little"))
        if _fq_gt_neg(P[1], q):
            b[-1] |= 1 << 7
        return bytes(b)
    if P is None:
        b = bytearray(2 * nb)
        b[0] |= 0x40
        return bytes(b)
    return P[0].to_bytes(nb, "big") + P[1].to_bytes(nb, "big")


def g2_uncompressed(curve: CurveParams, P) -> bytes:
    q, nb = curve.q, curve.fq_bytes
    if curve.bn_like:
        if P is None:
            b = bytearray(4 * nb)
            b[-1] |= 1 << 6
            return bytes(b)
        b = bytearray(b"".join(v.to_bytes(nb, "little") for v in (P[0][0], P[0][1], P[1][0], P[1][1])))
        if _fq2_gt_neg(P[1], q):
            b[-1] |= 1 << 7
        return bytes(b)
    if P is None:
        b = bytearray(4 * nb)
        b[0] |= 0x40
        return bytes(b)
    return b"".join(v.to_bytes(nb, "big") for v in (P[0][1], P[0][0], P[1][1], P[1][0]))


# ---- decoders (the specification: include/ark355.h, "ark-serialize wire formats") ------------------------------------------
# What a reader of these formats must hand back or refuse, in Python integers.  The order of the checks is part of the
# specification, because it decides the status of an encoding with several defects: flags, then reduction of every
# coordinate, then the curve equation, then the subgroup.
NOT_REDUCED, NOT_ON_CURVE, BAD_FLAGS, NOT_IN_SUBGROUP = 1, 2, 3, 4
STATUS_NAMES = {NOT_REDUCED: "not reduced", NOT_ON_CURVE: "not on curve", BAD_FLAGS: "bad flags",
                NOT_IN_SUBGROUP: "not in subgroup"}
VALIDATE_NONE, VALIDATE_FULL, VALIDATE_CURVE = 0, 1, 2


class WireError(ValueError):
    def __init__(self, status):
        self.status = status
        super().__init__(STATUS_NAMES[status])


def fq_sqrt(curve: CurveParams, v):
    """Square root in F_q for q = 3 mod 4 (both curves), or None."""
    q = curve.q
    assert q % 4 == 3
    v %= q
    r = pow(v, (q + 1) // 4, q)
    return r if r * r % q == v else None


def fq2_sqrt(curve: CurveParams, a):
    """Square root in F_q2 = F_q[u]/(u^2 + 1) for q = 3 mod 4 (both curves), or None."""
    q = curve.q
    a0, a1 = a[0] % q, a[1] % q
    if a1 == 0:
        r = fq_sqrt(curve, a0)
        if r is not None:
            return (r, 0)
        r = fq_sqrt(curve, -a0 % q)
        return None if r is None else (0, r)
    s = fq_sqrt(curve, (a0 * a0 + a1 * a1) % q)
    if s is None:
        return None
    inv2 = pow(2, -1, q)
    for t in ((a0 + s) * inv2 % q, (a0 - s) * inv2 % q):
        x0 = fq_sqrt(curve, t)
        if x0 is None or x0 == 0:
            continue
        x1 = a1 * pow(2 * x0, -1, q) % q
        if ((x0 * x0 - x1 * x1) % q, 2 * x0 * x1 % q) == (a0, a1):
            return (x0, x1)
    return None


def has_order_dividing_r(group, P, r) -> bool:
    """[r]P == O by plain double-and-add (Group.mul reduces its scalar mod r and cannot answer this)."""
    F = group.F
    acc = (F.one, F.one, F.zero)
    J = group.to_jac(P)
    for bit in bin(r)[2:]:
        acc = group.jdouble(acc)
        if bit == "1":
            acc = group.jadd(acc, J)
    return F.is_zero(acc[2])


def _decode(curve: CurveParams, group: int, data: bytes, compressed: bool, validate: int):
    q, nb = curve.q, curve.fq_bytes
    ncoord = group * (1 if compressed else 2)
    if len(data) != ncoord * nb:
        raise ValueError("an encoded point of %d bytes, not %d" % (ncoord * nb, len(data)))
    if validate not in (VALIDATE_NONE, VALIDATE_FULL, VALIDATE_CURVE):
        raise ValueError("validate")
    if curve.bn_like:
        # SWFlags in the two top bits of the last byte; both set is no flag value
        sign, inf = bool(data[-1] & 0x80), bool(data[-1] & 0x40)
        if sign and inf:
            raise WireError(BAD_FLAGS)
        body = data[:-1] + bytes([data[-1] & 0x3F])
        coords = [int.from_bytes(body[k * nb:(k + 1) * nb], "little") for k in range(ncoord)]
    else:
        # zcash flags in the three top bits of the first byte
        cbit, inf, sign = bool(data[0] & 0x80), bool(data[0] & 0x40), bool(data[0] & 0x20)
        if cbit != bool(compressed) or (sign and (inf or not compressed)):
            raise WireError(BAD_FLAGS)
        body = bytes([data[0] & 0x1F]) + data[1:]
        coords = [int.from_bytes(body[k * nb:(k + 1) * nb], "big") for k in range(ncoord)]
        if inf and any(body):
            raise WireError(BAD_FLAGS)                       # a payload under the infinity flag
    if any(c >= q for c in coords):
        raise WireError(NOT_REDUCED)
    if inf:
        return None                                          # BN254: a reduced payload is parsed and ignored
    if group == 1:
        G, x, root = _g1(curve), coords[0], fq_sqrt
        y = None if compressed else coords[1]
        gt_neg = _fq_gt_neg
    else:
        G, root, gt_neg = _g2(curve), fq2_sqrt, _fq2_gt_neg
        # element order on the wire: BLS12-381 c1 || c0, BN254 c0 || c1
        pair = (lambda a, b: (a, b)) if curve.bn_like else (lambda a, b: (b, a))
        x = pair(coords[0], coords[1])
        y = None if compressed else pair(coords[2], coords[3])
    F = G.F
    if compressed:
        y = root(curve, F.add(F.mul(F.sqr(x), x), G.b))
        if y is None:
            raise WireError(NOT_ON_CURVE)
        if gt_neg(y, q) != sign:
            y = F.neg(y)
    elif validate != VALIDATE_NONE and not G.is_on_curve((x, y)):
        raise WireError(NOT_ON_CURVE)                        # (BN254: the sign bit of this form is not looked at)
    P = (x, y)
    cofactor_one = curve.bn_like and group == 1
    if validate == VALIDATE_FULL and not cofactor_one and not has_order_dividing_r(G, P, curve.r):
        raise WireError(NOT_IN_SUBGROUP)
    return P


def g1_decode(curve: CurveParams, data: bytes, compressed: bool, validate: int = VALIDATE_FULL):
    """The point (None = infinity) of one encoded G1 point, or WireError with the status of its first defect."""
    return _decode(curve, 1, bytes(data), compressed, validate)


def g2_decode(curve: CurveParams, data: bytes, compressed: bool, validate: int = VALIDATE_FULL):
    return _decode(curve, 2, bytes(data), compressed, validate)


def verdict(curve: CurveParams, group: int, data: bytes, compressed: bool, validate: int):
    """(status, point): status 0 and the decoded point, or the refusal's status and None."""
    try:
        return 0, _decode(curve, group, bytes(data), compressed, validate)
    except WireError as e:
        return e.status, None


def proof_bytes(curve: CurveParams, proof, compressed=True) -> bytes:
    if compressed:
        return g1_compressed(curve, proof.a) + g2_compressed(curve, proof.b) + g1_compressed(curve, proof.c)
    return g1_uncompressed(curve, proof.a) + g2_uncompressed(curve, proof.b) + g1_uncompressed(curve, proof.c)


def _vec(items, enc):
    return len(items).to_bytes(8, "little") + b"".join(enc(x) for x in items)


def vk_bytes(curve, vk, compressed=True) -> bytes:
    e1 = (lambda P: g1_compressed(curve, P)) if compressed else (lambda P: g1_uncompressed(curve, P))
    e2 = (lambda P: g2_compressed(curve, P)) if compressed else (lambda P: g2_uncompressed(curve, P))
    return e1(vk.alpha_g1) + e2(vk.beta_g2) + e2(vk.gamma_g2) + e2(vk.delta_g2) + _vec(vk.gamma_abc_g1, e1)


def pk_bytes(curve, pk, compressed=False) -> bytes:
    e1 = (lambda P: g1_compressed(curve, P)) if compressed else (lambda P: g1_uncompressed(curve, P))
    e2 = (lambda P: g2_compressed(curve, P)) if compressed else (lambda P: g2_uncompressed(curve, P))
    return (vk_bytes(curve, pk.vk, compressed) + e1(pk.beta_g1) + e1(pk.delta_g1)
            + _vec(pk.a_query, e1) + _vec(pk.b_g1_query, e1) + _vec(pk.b_g2_query, e2)
            + _vec(pk.h_query, e1) + _vec(pk.l_query, e1))


# ---- raw memory images handed across the C ABI (include/ark355.h) --------------------------------
def g1_raw(curve: CurveParams, P) -> bytes:
    """x || y, LE u64 limbs, Montgomery form; infinity = all zero."""
    nb, q = curve.fq_bytes, curve.q
    if P is None:
        return bytes(2 * nb)
    R = 1 << (8 * nb)
    return (P[0] * R % q).to_bytes(nb, "little") + (P[1] * R % q).to_bytes(nb, "little")


def g2_raw(curve: CurveParams, P) -> bytes:
    """x.c0 || x.c1 || y.c0 || y.c1, Montgomery; infinity = all zero."""
    nb, q = curve.fq_bytes, curve.q
    if P is None:
        return bytes(4 * nb)
    R = 1 << (8 * nb)
    return b"".join((v * R % q).to_bytes(nb, "little") for v in (P[0][0], P[0][1], P[1][0], P[1][1]))


def g1_from_raw(curve: CurveParams, b: bytes):
    nb, q = curve.fq_bytes, curve.q
    if not any(b):
        return None
    Ri = pow(1 << (8 * nb), -1, q)
    return (int.from_bytes(b[:nb], "little") * Ri % q, int.from_bytes(b[nb:2 * nb], "little") * Ri % q)


def g2_from_raw(curve: CurveParams, b: bytes):
    nb, q = curve.fq_bytes, curve.q
    if not any(b):
        return None
    Ri = pow(1 << (8 * nb), -1, q)
    v = [int.from_bytes(b[i * nb:(i + 1) * nb], "little") * Ri % q for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def fr_mont(curve: CurveParams, v) -> bytes:
    nb = curve.fr_bytes
    return (v % curve.r * (1 << (8 * nb)) % curve.r).to_bytes(nb, "little")


def fr_canon(curve: CurveParams, v) -> bytes:
    return (v % curve.r).to_bytes(curve.fr_bytes, "little")


def fr_from_mont(curve: CurveParams, b: bytes) -> int:
    nb = curve.fr_bytes
    return int.from_bytes(b, "little") * pow(1 << (8 * nb), -1, curve.r) % curve.r
