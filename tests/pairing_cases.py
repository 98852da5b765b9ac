"""Pairing cases shared by the CPU-emulator tier (test_emul_pairing.py) and the GPU tier (test_gpu_pairing.py): each drives
`ark355_multi_pairing` / `ark355_verify_batch` through `snark_amd._binding.Lib` and compares with oracle/pairing.py.

The oracle costs one pairing per curve (cached) plus one power in GT per case, whatever the number of pairs: the pairs have
known discrete logarithms, P_i = a_i G1 and Q_i = b_i G2, so prod e(P_i, Q_i) = e(G1, G2)^(sum a_i b_i)."""
from __future__ import annotations

import random

import pytest

from helpers import g1_vec_raw, z_bytes
from oracle import groth16 as G, serialize as Z, synthetic as S
from oracle.curves import g1, g2
from oracle.pairing import Pairing
from oracle.serialize import fq2_sqrt

_PAIRING = {}
_E = {}


def pairing_of(C):
    if C.name not in _PAIRING:
        _PAIRING[C.name] = Pairing(C)
    return _PAIRING[C.name]


def e_of_generators(C):
    """e(G1, G2) of the oracle (for BLS12-381 the oracle ignores the sign of x: this is the INVERSE of the real pairing)."""
    if C.name not in _E:
        _E[C.name] = pairing_of(C).pairing(g1(C).gen, g2(C).gen)
    return _E[C.name]


def gt_to_flat(C, gt: bytes):
    """12 Fq in ark-ff's Fp12 order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1; Montgomery) -> the oracle's flat basis
    1, w, ..., w^11: the coefficient a + b u of v^j w^i goes to (a - k b) w^(2j+i) + b w^(2j+i+6), k = 1 / 9."""
    nb, q = C.fq_bytes, C.q
    assert len(gt) == 12 * nb
    Ri = pow(1 << (8 * nb), -1, q)
    v = [int.from_bytes(gt[t * nb:(t + 1) * nb], "little") * Ri % q for t in range(12)]
    k = 9 if C.bn_like else 1
    out = [0] * 12
    for i in range(2):
        for j in range(3):
            a, b = v[i * 6 + j * 2], v[i * 6 + j * 2 + 1]
            out[2 * j + i] = (out[2 * j + i] + a - k * b) % q
            out[2 * j + i + 6] = (out[2 * j + i + 6] + b) % q
    return out


def expected_gt(C, exponent):
    """e(G1, G2)^exponent as the LIBRARY defines it, in the oracle's basis."""
    F = pairing_of(C).F
    e = exponent % C.r
    if not C.bn_like:
        e = (C.r - e) % C.r              # oracle/pairing.py computes e(P, Q)^-1 on BLS12-381 (its docstring)
    return F.pow(e_of_generators(C), e)


def points_with_dlogs(lib, ctx, C, a, b, cross_check=3):
    """P_i = a_i G1, Q_i = b_i G2 from ark355_fixed_base_mul; the first `cross_check` of each against the oracle's own."""
    sz = lib.sizes(C.curve_id)
    G1, G2 = g1(C), g2(C)
    n = len(a)
    p = lib.fixed_base_mul(ctx, C.curve_id, 1, Z.g1_raw(C, G1.gen), b"".join(Z.fr_canon(C, x) for x in a), n, sz["g1"])
    q = lib.fixed_base_mul(ctx, C.curve_id, 2, Z.g2_raw(C, G2.gen), b"".join(Z.fr_canon(C, x) for x in b), n, sz["g2"])
    for i in range(min(cross_check, n)):
        assert p[i * sz["g1"]:(i + 1) * sz["g1"]] == Z.g1_raw(C, G1.mul(G1.gen, a[i] % C.r))
        assert q[i * sz["g2"]:(i + 1) * sz["g2"]] == Z.g2_raw(C, G2.mul(G2.gen, b[i] % C.r))
    return p, q


def mixed_scalars(C, n, seed):
    """Random discrete logs with 0 (a point at infinity on either side), 1, r - 1 and a repeated pair mixed in as n allows."""
    rnd = random.Random(seed * 7919 + n)
    a = [rnd.randrange(1, C.r) for _ in range(n)]
    b = [rnd.randrange(1, C.r) for _ in range(n)]
    if n >= 2:
        a[1] = C.r - 1
    if n >= 3:
        b[2] = 1
    if n >= 4:
        a[3], b[3] = a[0], b[0]                 # repeated pair
    if n >= 8:
        a[4] = 0                                # P at infinity
        b[5] = 0                                # Q at infinity
        a[6], b[6] = 1, C.r - 1
        a[7], b[7] = 0, 0
    return a, b


def gt_case(lib, ctx, C, n, seed=41, points=None):
    """out_gt against e(G1, G2)^(sum a_i b_i); is_one after appending (-(sum a_i b_i) G1, G2), and not with a scalar off by one.
    points: (a, b, g1 bytes, g2 bytes) made earlier (the large cases are generated once per session)."""
    sz = lib.sizes(C.curve_id)
    if points is None:
        a, b = mixed_scalars(C, n, seed)
        points = (a, b) + points_with_dlogs(lib, ctx, C, a, b)
    a, b, p, q = points
    assert len(a) == n
    s = sum(x * y for x, y in zip(a, b)) % C.r
    gt, one = lib.multi_pairing(ctx, C.curve_id, p, q, n)
    F = pairing_of(C).F
    assert F.eq(gt_to_flat(C, gt), expected_gt(C, s)), (C.name, n)
    assert one == (s == 0)
    # closing pair: prod e(P_i, Q_i) e(-s G1, G2) = 1
    G1, G2 = g1(C), g2(C)
    close = Z.g1_raw(C, G1.mul(G1.gen, (C.r - s) % C.r))
    off = Z.g1_raw(C, G1.mul(G1.gen, (C.r - s + 1) % C.r))
    gen2 = Z.g2_raw(C, G2.gen)
    gt1, one1 = lib.multi_pairing(ctx, C.curve_id, p + close, q + gen2, n + 1)
    assert one1 and F.eq(gt_to_flat(C, gt1), F.one)
    _, one2 = lib.multi_pairing(ctx, C.curve_id, p + off, q + gen2, n + 1, want_gt=False)
    assert not one2
    assert len(gt) == 12 * sz["fq"]


def routes_agree_case(lib, ctx, policy, C, n, seed=43):
    """PAIRING_DEVICE=0 (host threads) and =1 (device) give byte-equal GT: pins the device loop to the host loop after the
    final exponentiation (raw Miller values may differ by subfield factors and are not compared)."""
    a, b = mixed_scalars(C, n, seed)
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=1)
    policy.setenv("ARK355_PAIRING_DEVICE", 0)
    host = lib.multi_pairing(ctx, C.curve_id, p, q, n)
    policy.setenv("ARK355_PAIRING_DEVICE", 1)
    dev = lib.multi_pairing(ctx, C.curve_id, p, q, n)
    assert host == dev, (C.name, n)
    assert any(host[0])


def lines_case(lib, ctx, C, m, seed=47):
    """m random pairs (P, Q), each followed by (-P, Q): the product is one.  The library's verdict against the oracle's
    pairing_product_is_one on the same list, and on the list with one pair perturbed."""
    rnd = random.Random(seed + m)
    G1, G2 = g1(C), g2(C)
    Ps = G1.fixed_base_muls(G1.gen, [rnd.randrange(1, C.r) for _ in range(m)])
    Qs = G2.fixed_base_muls(G2.gen, [rnd.randrange(1, C.r) for _ in range(m)])
    pairs = []
    for P, Q in zip(Ps, Qs):
        pairs += [(P, Q), (G1.neg(P), Q)]

    def verdict(prs):
        _, one = lib.multi_pairing(ctx, C.curve_id, b"".join(Z.g1_raw(C, P) for P, _ in prs),
                                   b"".join(Z.g2_raw(C, Q) for _, Q in prs), len(prs), want_gt=False)
        return one

    O = pairing_of(C)
    assert verdict(pairs) is True and O.pairing_product_is_one(pairs) is True
    bad = list(pairs)
    k = (2 * m) // 2 + 1 if m > 1 else 1
    bad[k] = (G1.add(bad[k][0], G1.gen), bad[k][1])
    assert verdict(bad) == O.pairing_product_is_one(bad) == False       # noqa: E712


def non_subgroup_g2(C, seed=53):
    """A point of the twist outside the r-torsion: pick x, solve for y (the cofactor of G2 is huge, so the first x works)."""
    G2 = g2(C)
    F = G2.F
    rnd = random.Random(seed)
    while True:
        x = (rnd.randrange(C.q), rnd.randrange(C.q))
        y = fq2_sqrt(C, F.add(F.mul(F.sqr(x), x), G2.b))
        if y is None:
            continue
        P = (x, y)
        assert G2.is_on_curve(P)
        if G2.add(G2.mul(P, C.r - 1), P) is not None:          # r P != 0 (Group.mul reduces its scalar mod r)
            return P


def refusals_case(lib, ctx, C, err_type, einval, n=5):
    """Off-curve points at a middle index are refused by name, n = 0 is accepted, NULL with n > 0 is refused, a point on the
    twist outside the subgroup returns cleanly."""
    sz = lib.sizes(C.curve_id)
    a, b = mixed_scalars(C, n, seed=59)
    a[1], b[2] = 7, 9
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=0)
    mid = n // 2

    def poke(buf, size, idx):
        raw = bytearray(buf)
        raw[idx * size + size // 2] ^= 1          # lowest byte of y (of y.c0 in G2): still reduced, no longer on the curve
        return bytes(raw)

    for which, (pp, qq) in (("g1", (poke(p, sz["g1"], mid), q)), ("g2", (p, poke(q, sz["g2"], mid)))):
        with pytest.raises(err_type) as e:
            lib.multi_pairing(ctx, C.curve_id, pp, qq, n)
        assert e.value.code == einval and "%s[%d]" % (which, mid) in str(e.value), str(e.value)
    gt, one = lib.multi_pairing(ctx, C.curve_id, b"", b"", 0)
    assert one and pairing_of(C).F.eq(gt_to_flat(C, gt), pairing_of(C).F.one)
    with pytest.raises(err_type) as e:
        lib.multi_pairing(ctx, C.curve_id, b"", q, n)
    assert e.value.code == einval
    # on the twist, outside the subgroup: a clean return, whatever the value
    X = non_subgroup_g2(C)
    qq = bytearray(q)
    qq[mid * sz["g2"]:(mid + 1) * sz["g2"]] = Z.g2_raw(C, X)
    gt, one = lib.multi_pairing(ctx, C.curve_id, p, bytes(qq), n)
    assert len(gt) == 12 * sz["fq"] and one in (True, False)


def oracle_batch(C, count, n=9, seed=61):
    """`count` proofs of one oracle-made key: (vk parts, [(a, b, c) raw], [public input bytes], [z])."""
    rnd = random.Random(seed)
    td = G.Trapdoor(tau=rnd.randrange(2, C.r), alpha=3, beta=5, gamma=7, delta=11)
    A, B, Cm, z0, ell = S.mulchain_direct(C.r, n, seed=seed)
    pk = G.setup(C, A, B, Cm, ell, len(z0), td)
    vk = (Z.g1_raw(C, pk.vk.alpha_g1), Z.g2_raw(C, pk.vk.beta_g2), Z.g2_raw(C, pk.vk.gamma_g2), Z.g2_raw(C, pk.vk.delta_g2),
          g1_vec_raw(C, pk.vk.gamma_abc_g1))
    proofs, inputs, zs = [], [], []
    for j in range(count):
        _, _, _, z, _ = S.mulchain_direct(C.r, n, seed=seed + 1 + j)
        p = G.prove_closed_form(C, pk, z, ell, rnd.randrange(C.r), rnd.randrange(C.r))
        proofs.append((Z.g1_raw(C, p.a), Z.g2_raw(C, p.b), Z.g1_raw(C, p.c)))
        inputs.append(z_bytes(C, z[1:ell]))
        zs.append(z)
    return vk, proofs, inputs, zs, ell


def large_batch_case(lib, ctx, C, batch, total=4096, tamper=4000):
    """A batch of `total` proofs built by cycling the oracle-made ones with distinct rho: accepts; rejects with one proof
    tampered at index `tamper`, with one wrong public input, and with A at infinity."""
    vk, proofs, inputs, zs, ell = batch
    k = len(proofs)
    rnd = random.Random(67)
    ps = [proofs[j % k] for j in range(total)]
    xs = [inputs[j % k] for j in range(total)]
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(total)]
    assert len(set(rho)) == total
    assert lib.verify_batch(ctx, C.curve_id, vk, ps, b"".join(xs), rho)
    bad = list(ps)
    other = proofs[(tamper + 1) % k]
    bad[tamper] = (ps[tamper][0], ps[tamper][1], other[2])
    assert not lib.verify_batch(ctx, C.curve_id, vk, bad, b"".join(xs), rho)
    wrong = list(xs)
    wrong[tamper // 2] = z_bytes(C, [(zs[(tamper // 2) % k][1] + 1) % C.r] + list(zs[(tamper // 2) % k][2:ell]))
    assert not lib.verify_batch(ctx, C.curve_id, vk, ps, b"".join(wrong), rho)
    inf = list(ps)
    inf[tamper] = (bytes(len(ps[0][0])), ps[tamper][1], ps[tamper][2])
    assert not lib.verify_batch(ctx, C.curve_id, vk, inf, b"".join(xs), rho)
