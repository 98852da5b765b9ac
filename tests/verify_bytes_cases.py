"""Proofs as wire bytes: cases shared by the CPU-emulator tier (test_emul_verify_bytes.py) and the GPU tier
(test_gpu_verify_bytes.py) for `ark355_points_check`, `ark355_proofs_from_bytes` and `ark355_verify_each_bytes`, through
`snark_amd._binding.Lib`.

The reference is never the code under test: statuses and decoded points come from the oracle's own decoder
(`oracle.serialize.verdict`, `has_order_dividing_r`, `is_on_curve`), the bytes from the oracle's encoders, and the verdicts of
the malleability case from `oracle.groth16.verify`.  For the proofs that decode, the pairing verdict is the one
`ark355_verify_each_pvk` gives on the oracle-decoded points (that entry has its own tests against the oracle).

Oracle work is cached per process: the verdict of an encoded point by its bytes, the point mixes by curve and group."""
from __future__ import annotations

import ctypes
import random

from helpers import g1_vec_raw, z_bytes
from oracle import groth16 as G, serialize as Z, synthetic as S
from oracle.curves import g1, g2
from pvk_cases import each_chunk_proofs, processed
from pairing_cases import points_with_dlogs
from pairing_each_cases import tampered_batch

NONE, FULL, CURVE = Z.VALIDATE_NONE, Z.VALIDATE_FULL, Z.VALIDATE_CURVE
MODES = (NONE, CURVE, FULL)
BLS_X = 0xd201000000010000


# ---- points ----------------------------------------------------------------------------------------------------------------
def group_of(C, group):
    return g1(C) if group == 1 else g2(C)


def plain_mul(G_, P, k):
    """[k]P by plain double-and-add: Group.mul reduces its scalar mod r, which is wrong outside the subgroup."""
    F = G_.F
    acc = (F.one, F.one, F.zero)
    if P is None or k == 0:
        return None
    J = G_.to_jac(P)
    for bit in bin(k)[2:]:
        acc = G_.jdouble(acc)
        if bit == "1":
            acc = G_.jadd(acc, J)
    return G_.to_affine(acc)


def cofactor(C, group):
    """#E / r from the curve families' parameterisations (checked against r below)."""
    if C.bn_like:
        h = 1 if group == 1 else 2 * C.q - C.r
    else:
        x = -BLS_X
        h = (x - 1) ** 2 // 3 if group == 1 else (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    return h


def random_curve_point(C, group, rnd):
    """A random point of the whole curve group: pick x, solve for y (as pairing_cases.non_subgroup_g2 does for G2)."""
    G_ = group_of(C, group)
    F = G_.F
    while True:
        x = rnd.randrange(C.q) if group == 1 else (rnd.randrange(C.q), rnd.randrange(C.q))
        rhs = F.add(F.mul(F.sqr(x), x), G_.b)
        y = Z.fq_sqrt(C, rhs) if group == 1 else Z.fq2_sqrt(C, rhs)
        if y is not None:
            assert G_.is_on_curve((x, y))
            return (x, y)


def off_curve(C, group):
    G_ = group_of(C, group)
    x, y = G_.gen
    bad = (x, (y + 1) % C.q) if group == 1 else (x, ((y[0] + 1) % C.q, y[1]))
    assert not G_.is_on_curve(bad)
    return bad


def to_raw(C, group, P):
    return Z.g1_raw(C, P) if group == 1 else Z.g2_raw(C, P)


_MIX = {}


def point_mix(C, group):
    """[(point, expected status)]: the generator, small multiples, infinity, random curve points, cofactor-cleared points [h]P,
    pure cofactor torsion [r]P, mixed [r]P + [h]P', a point off the curve.  The expectation is the oracle's is_on_curve /
    has_order_dividing_r; the construction is asserted to give both verdicts where the group has a cofactor."""
    key = (C.name, group)
    if key in _MIX:
        return _MIX[key]
    G_ = group_of(C, group)
    rnd = random.Random(211 + 2 * C.curve_id + group)
    h = cofactor(C, group)
    R1, R2, R3 = (random_curve_point(C, group, rnd) for _ in range(3))
    cleared, cleared2 = plain_mul(G_, R1, h), plain_mul(G_, R3, h)
    torsion = plain_mul(G_, R2, C.r)
    pts = [G_.gen, G_.mul(G_.gen, 2), G_.mul(G_.gen, 3), None, R1, R2, cleared, torsion, G_.add(torsion, cleared2),
           off_curve(C, group), G_.mul(G_.gen, C.r - 1), G_.neg(R3)]
    assert plain_mul(G_, cleared, C.r) is None, "the cofactor does not clear: wrong h"
    out = []
    for P in pts:
        if not G_.is_on_curve(P):
            out.append((P, Z.NOT_ON_CURVE))
        else:
            out.append((P, 0 if P is None or Z.has_order_dividing_r(G_, P, C.r) else Z.NOT_IN_SUBGROUP))
    want = [s for _, s in out]
    if C.bn_like and group == 1:
        assert want.count(0) == len(pts) - 1 and torsion is None          # cofactor 1: every curve point is in the group
    else:
        assert want[4] == want[5] == want[7] == want[8] == want[11] == Z.NOT_IN_SUBGROUP and want[6] == 0
    _MIX[key] = out
    return out


def points_check_case(lib, ctx, C, group, n):
    """status under the endomorphism tests == status under [r]P == the oracle's, for n points cycling the mix from a rotating
    start (so that every kind meets the ends of a wave and the second workgroup)."""
    mix = point_mix(C, group)
    sel = [mix[(i + n) % len(mix)] for i in range(n)]
    raw = b"".join(to_raw(C, group, P) for P, _ in sel)
    want = [s for _, s in sel]
    slow = lib.points_check(ctx, C.curve_id, group, raw, n, method=0)
    fast = lib.points_check(ctx, C.curve_id, group, raw, n, method=1)
    assert slow == want, (C.name, group, n, "[r]P", [i for i in range(n) if slow[i] != want[i]][:8])
    assert fast == want, (C.name, group, n, "endomorphism", [i for i in range(n) if fast[i] != want[i]][:8])


# ---- proofs and their encodings --------------------------------------------------------------------------------------------
_BATCH = {}


def oracle_proofs(C, count=8, n=9, seed=61):
    """(batch, vk object, [Proof], [public inputs]): pairing_cases.oracle_batch's construction, keeping the oracle's objects
    next to the raw images (batch is the tuple oracle_batch returns, for pairing_each_cases.tampered_batch)."""
    key = (C.name, count)
    if key in _BATCH:
        return _BATCH[key]
    rnd = random.Random(seed)
    td = G.Trapdoor(tau=rnd.randrange(2, C.r), alpha=3, beta=5, gamma=7, delta=11)
    A, B, Cm, z0, ell = S.mulchain_direct(C.r, n, seed=seed)
    pk = G.setup(C, A, B, Cm, ell, len(z0), td)
    vk = (Z.g1_raw(C, pk.vk.alpha_g1), Z.g2_raw(C, pk.vk.beta_g2), Z.g2_raw(C, pk.vk.gamma_g2), Z.g2_raw(C, pk.vk.delta_g2),
          g1_vec_raw(C, pk.vk.gamma_abc_g1))
    objs, proofs, inputs, zs = [], [], [], []
    for j in range(count):
        _, _, _, z, _ = S.mulchain_direct(C.r, n, seed=seed + 1 + j)
        p = G.prove_closed_form(C, pk, z, ell, rnd.randrange(C.r), rnd.randrange(C.r))
        objs.append(p)
        proofs.append((Z.g1_raw(C, p.a), Z.g2_raw(C, p.b), Z.g1_raw(C, p.c)))
        inputs.append(z_bytes(C, z[1:ell]))
        zs.append(z)
    _BATCH[key] = ((vk, proofs, inputs, zs, ell), pk.vk, objs, [list(z[1:ell]) for z in zs])
    return _BATCH[key]


def encode(C, group, P, comp):
    if group == 1:
        return Z.g1_compressed(C, P) if comp else Z.g1_uncompressed(C, P)
    return Z.g2_compressed(C, P) if comp else Z.g2_uncompressed(C, P)


def sizes_of(C, comp):
    s1, s2 = C.fq_bytes * (1 if comp else 2), C.fq_bytes * (2 if comp else 4)
    return s1, s2, 2 * s1 + s2


def split(C, wire, comp):
    s1, s2, _ = sizes_of(C, comp)
    return [wire[:s1], wire[s1:s1 + s2], wire[s1 + s2:]]


_VERDICT = {}


def verdict(C, group, enc, comp, mode):
    key = (C.name, group, bytes(enc), comp, mode)
    if key not in _VERDICT:
        _VERDICT[key] = Z.verdict(C, group, enc, comp, mode)
    return _VERDICT[key]


def expected(C, wire, comp, mode):
    """(status, (a, b, c) raw images) of one encoded proof from the oracle's decoder: the status of the FIRST failing point in
    the order a, b, c with its position in the high nibble, and all-zero images where it is not 0."""
    n1, n2 = 2 * C.fq_bytes, 4 * C.fq_bytes
    pts = []
    for k, (group, enc) in enumerate(zip((1, 2, 1), split(C, wire, comp))):
        st, P = verdict(C, group, enc, comp, mode)
        if st:
            return ((k + 1) << 4) | st, (bytes(n1), bytes(n2), bytes(n1))
        pts.append(to_raw(C, group, P))
    return 0, tuple(pts)


def _set_x(C, group, enc, value):
    """The first base-field element of the encoding replaced by `value`, flag bits kept."""
    nb = C.fq_bytes
    b = bytearray(enc)
    if C.bn_like:
        # c0 of G2 / x of G1 is the first element and carries no flags unless it is also the last one (compressed G1)
        b[:nb] = value.to_bytes(nb, "little")
        if len(b) == nb:
            b[-1] |= enc[-1] & 0xC0
    else:
        b[:nb] = value.to_bytes(nb, "big")
        b[0] |= enc[0] & 0xE0
    return bytes(b)


def damages(C, group, comp):
    """[(name, encoded point)] for one group and form: every kind of defect the decoders must tell apart, and the legal
    encodings next to them (infinity; on BN254 a reduced payload under the infinity flag)."""
    G_ = group_of(C, group)
    rnd = random.Random(223 + group)
    good = encode(C, group, G_.mul(G_.gen, 5), comp)
    size = len(good)
    out = [("x = q", _set_x(C, group, good, C.q)), ("x = 2^bits - 1", _set_x(C, group, good, (1 << (C.q.bit_length())) - 1))]
    inf = encode(C, group, None, comp)
    if C.bn_like:
        both = bytearray(good)
        both[-1] |= 0xC0
        out.append(("both flag bits", bytes(both)))
        pay = bytearray(inf)
        pay[0] = 1
        out.append(("reduced payload under the infinity flag (legal)", bytes(pay)))
        big = bytearray(_set_x(C, group, inf, C.q))
        out.append(("unreduced payload under the infinity flag", bytes(big)))
    else:
        wrong_c = bytearray(good)
        wrong_c[0] ^= 0x80
        out.append(("compressed bit of the other form", bytes(wrong_c)))
        si = bytearray(inf)
        si[0] |= 0x20
        out.append(("sort bit with infinity", bytes(si)))
        if not comp:
            so = bytearray(good)
            so[0] |= 0x20
            out.append(("sort bit without the compressed bit", bytes(so)))
        pay = bytearray(inf)
        pay[-1] = 1
        out.append(("payload under the infinity flag", bytes(pay)))
    if comp:
        F = G_.F
        while True:
            x = rnd.randrange(C.q) if group == 1 else (rnd.randrange(C.q), rnd.randrange(C.q))
            rhs = F.add(F.mul(F.sqr(x), x), G_.b)
            if (Z.fq_sqrt(C, rhs) if group == 1 else Z.fq2_sqrt(C, rhs)) is None:
                break
        out.append(("x with no square root", encode(C, group, (x, G_.gen[1]), True)))
    else:
        out.append(("off the curve", encode(C, group, off_curve(C, group), False)))
    out.append(("outside the subgroup", encode(C, group, point_mix(C, group)[4][0], comp)))
    out.append(("cofactor torsion", encode(C, group, point_mix(C, group)[7][0], comp)))
    out.append(("infinity (legal)", inf))
    assert all(len(e) == size for _, e in out)
    return out


def proof_wires(C, comp, count):
    """`count` encoded proofs cycling the oracle's, every second one damaged in one point: the kinds of damages() in the
    positions a, b, c in turn, so the neighbours of a damaged proof are always whole.  -> (list of wires, number damaged)"""
    _, _, objs, _ = oracle_proofs(C)
    wires = [Z.proof_bytes(C, objs[j % len(objs)], comp) for j in range(count)]
    plan = [(pos, d) for pos in range(3) for d in damages(C, 2 if pos == 1 else 1, comp)]
    # two defects in one proof: the FIRST in the order a, b, c decides
    done = 0
    for j in range(1, count, 2):
        pos, (_, enc) = plan[(j // 2) % len(plan)]
        parts = split(C, wires[j], comp)
        parts[pos] = enc
        if j % 8 == 7:
            parts[2] = damages(C, 1, comp)[0][1]
        wires[j] = b"".join(parts)
        done += 1
    return wires, done


def decoder_case(lib, ctx, C, comp, mode, count):
    """ark355_proofs_from_bytes against the oracle's decoder, byte for byte and status for status."""
    sz = lib.sizes(C.curve_id)
    wires, _ = proof_wires(C, comp, count)
    want = [expected(C, w, comp, mode) for w in wires]
    got, status = lib.proofs_from_bytes(ctx, C.curve_id, b"".join(wires), count, sz, comp, mode)
    bad = [j for j in range(count) if status[j] != want[j][0]]
    assert not bad, (C.name, comp, mode, [(j, status[j], want[j][0]) for j in bad[:8]])
    assert got == [w[1] for w in want], (C.name, comp, mode, [j for j in range(count) if got[j] != want[j][1]][:8])
    if count >= 43:                       # the plan covers every kind: every status value occurs, and so do whole proofs
        seen = {s & 15 for s in status}
        assert {0, Z.NOT_REDUCED, Z.BAD_FLAGS} <= seen and {s >> 4 for s in status} == {0, 1, 2, 3}
        assert (Z.NOT_IN_SUBGROUP in seen) == (mode == FULL)
        assert (Z.NOT_ON_CURVE in seen) == (comp or mode != NONE)


# ---- ark355_verify_each_bytes ------------------------------------------------------------------------------------------------
def raw_to_wire(C, proof, comp):
    a, b, c = proof
    return (encode(C, 1, Z.g1_from_raw(C, a), comp) + encode(C, 2, Z.g2_from_raw(C, b), comp) + encode(C, 1, Z.g1_from_raw(C, c), comp))


def reference(lib, ctx, C, h, wires, xs, comp, mode):
    """(ok, status): the oracle's decoder, then ark355_verify_each_pvk on the oracle-decoded points, AND status == 0."""
    dec = [expected(C, w, comp, mode) for w in wires]
    oks = lib.verify_each_pvk(ctx, h, [d[1] for d in dec], b"".join(xs))
    return [bool(o and d[0] == 0) for o, d in zip(oks, dec)], [d[0] for d in dec]


def verify_each_bytes_case(lib, ctx, policy, C, comp, mode, total, tamper=None, wire_damage=True):
    """ok and status exact on the device route and on the host route: pairing tampers (status 0, ok 0) and wire defects
    (status != 0, ok 0) next to whole proofs."""
    batch = oracle_proofs(C)[0]
    if tamper is None:
        tamper = dict(other_c=(0,), wrong_input=(63,), a_inf=(64,), b_off=(65,), swapped=(129,))
    tamper = {k: tuple(j for j in v if j < total) for k, v in tamper.items()}
    ps, xs, _ = tampered_batch(C, batch, total, **tamper)
    cache = {}
    wires = []
    for p in ps:
        if p not in cache:
            cache[p] = raw_to_wire(C, p, comp)
        wires.append(cache[p])
    tampered = {j for v in tamper.values() for j in v}
    if wire_damage:
        kinds = [(pos, d) for pos in range(3) for d in damages(C, 2 if pos == 1 else 1, comp)]
        free = [j for j in range(2, total, 3) if j not in tampered]
        for t, j in enumerate(free[:len(kinds)]):
            pos, (_, enc) = kinds[t]
            parts = split(C, wires[j], comp)
            parts[pos] = enc
            wires[j] = b"".join(parts)
    with processed(lib, ctx, C, batch[0]) as h:
        policy.setenv("ARK355_PAIRING_DEVICE", 1)
        want = reference(lib, ctx, C, h, wires, xs, comp, mode)
        for j in tampered - set(tamper.get("b_off", ())):      # (a poked y of B: whatever the oracle's decoder makes of its bytes;
            assert want[0][j] is False and want[1][j] == 0, j  # the compressed form carries only its sign)
        blob = b"".join(wires)
        for route in (1, 0):
            policy.setenv("ARK355_PAIRING_DEVICE", route)
            got = lib.verify_each_bytes(ctx, h, blob, total, b"".join(xs), comp, mode)
            assert got[1] == want[1], (C.name, comp, mode, route, [(j, got[1][j], want[1][j]) for j in range(total) if got[1][j] != want[1][j]][:8])
            assert got[0] == want[0], (C.name, comp, mode, route, [j for j in range(total) if got[0][j] != want[0][j]][:8])
            assert lib.verify_each_bytes(ctx, h, blob, total, b"".join(xs), comp, mode, want_status=False) == (want[0], None)
    if total >= 3:
        assert True in want[0] and False in want[0]


def past_the_chunk_case(lib, ctx, C, comp=True, mode=FULL):
    """One proof more than a chunk of the Miller stage holds, tiled from the oracle's, with a wire defect and a pairing tamper
    in the first and the last proof of every chunk."""
    batch, _, _, _ = oracle_proofs(C)
    total = each_chunk_proofs() + 1
    chunk = each_chunk_proofs()
    ends = sorted({j for c in range(0, total, chunk) for j in (c, min(c + chunk, total) - 1)})
    ps, xs, _ = tampered_batch(C, batch, total, other_c=ends[::2])
    base = {p: raw_to_wire(C, p, comp) for p in set(ps)}
    wires = [base[p] for p in ps]
    for j in ends[1::2]:
        parts = split(C, wires[j], comp)
        parts[1] = damages(C, 2, comp)[-3][1]                  # B outside the subgroup
        wires[j] = b"".join(parts)
    with processed(lib, ctx, C, batch[0]) as h:
        want = reference(lib, ctx, C, h, wires, xs, comp, mode)
        got = lib.verify_each_bytes(ctx, h, b"".join(wires), total, b"".join(xs), comp, mode)
    assert got[1] == want[1] and got[0] == want[0], (C.name, [j for j in range(total) if got[0][j] != want[0][j]][:8])
    assert want[0].count(False) == len(ends) and [want[1][j] for j in ends[1::2]] == [(2 << 4) | Z.NOT_IN_SUBGROUP] * len(ends[1::2])


def no_public_inputs_case(lib, ctx, C, comp=True):
    """num_instance == 1 with public_inputs NULL (the construction of pvk_cases.no_public_inputs_case)."""
    rnd = random.Random(89)
    a, b, s, x, y = (rnd.randrange(1, C.r) for _ in range(5))
    z = (x * y - a * b - s) % C.r
    g1s, g2s = points_with_dlogs(lib, ctx, C, [a, s, x, z, (z + 1) % C.r], [b, 1, y, 1, 1], cross_check=1)
    n1, n2 = lib.sizes(C.curve_id)["g1"], lib.sizes(C.curve_id)["g2"]
    P = [g1s[i * n1:(i + 1) * n1] for i in range(5)]
    Q = [g2s[i * n2:(i + 1) * n2] for i in range(5)]
    vk = (P[0], Q[0], Q[1], Q[1], P[1])
    wires = [raw_to_wire(C, (P[2], Q[2], P[3]), comp), raw_to_wire(C, (P[2], Q[2], P[4]), comp)]
    with processed(lib, ctx, C, vk) as h:
        assert lib.verify_each_bytes(ctx, h, b"".join(wires), 2, b"", comp, FULL) == ([True, False], [0, 0])


def malleability_case(lib, ctx, policy, C, comp):
    """A + T and C + T with T = [r]P of small order: the pairing cannot see T, so the oracle's verifier accepts both -- under
    VALIDATE_CURVE ok is the oracle's verdict on the same points; under VALIDATE_FULL each costs its proof a 0 with the
    status of the point that carries T."""
    assert not C.bn_like, "BN254's G1 has cofactor 1: there is no T"
    batch, vk_obj, objs, inputs = oracle_proofs(C)
    G1 = g1(C)
    T = point_mix(C, 1)[7][0]
    assert T is not None and Z.has_order_dividing_r(G1, T, cofactor(C, 1)) and not Z.has_order_dividing_r(G1, T, C.r)
    p = objs[0]
    cands = [G.Proof(G1.add(p.a, T), p.b, p.c), G.Proof(p.a, p.b, G1.add(p.c, T)), p]
    oracle_ok = [G.verify(C, vk_obj, inputs[0], q) for q in cands]
    assert oracle_ok == [True, True, True], oracle_ok           # the claim of include/ark355.h: many accepted encodings
    blob = b"".join(Z.proof_bytes(C, q, comp) for q in cands)
    xs = batch[2][0] * 3
    with processed(lib, ctx, C, batch[0]) as h:
        for route in (1, 0):
            policy.setenv("ARK355_PAIRING_DEVICE", route)
            assert lib.verify_each_bytes(ctx, h, blob, 3, xs, comp, CURVE) == (oracle_ok, [0, 0, 0]), (comp, route)
            want = ([False, False, True], [(1 << 4) | Z.NOT_IN_SUBGROUP, (3 << 4) | Z.NOT_IN_SUBGROUP, 0])
            assert lib.verify_each_bytes(ctx, h, blob, 3, xs, comp, FULL) == want, (comp, route)


def refusals_case(lib, ctx, C, einval):
    """Argument errors are ARK355_EINVAL and ark355_last_error names the argument; count = 0 and n = 0 write nothing; a bad
    proof is not an error of the call."""
    batch = oracle_proofs(C)[0]
    dll = lib.dll
    sz = lib.sizes(C.curve_id)
    wire = raw_to_wire(C, batch[1][0], True)
    buf = (ctypes.c_uint8 * len(wire)).from_buffer_copy(wire)
    xs = (ctypes.c_uint8 * len(batch[2][0])).from_buffer_copy(batch[2][0])
    ok = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    st = (ctypes.c_uint8 * 4)(9, 9, 9, 9)
    out = (ctypes.c_uint8 * (2 * (96 + 192 + 96)))()
    raw = (ctypes.c_uint8 * sz["g1"]).from_buffer_copy(batch[1][0][0])

    def refused(rc, word):
        msg = dll.ark355_last_error(ctx).decode()
        assert rc == einval and word in msg, (rc, word, msg)

    with processed(lib, ctx, C, batch[0]) as h:
        assert dll.ark355_verify_each_bytes(None, h, buf, 1, 1, FULL, xs, ok, st) == einval
        refused(dll.ark355_verify_each_bytes(ctx, None, buf, 1, 1, FULL, xs, ok, st), "pvk")
        refused(dll.ark355_verify_each_bytes(ctx, h, None, 1, 1, FULL, xs, ok, st), "proofs")
        refused(dll.ark355_verify_each_bytes(ctx, h, buf, 1, 1, FULL, xs, None, st), "ok")
        refused(dll.ark355_verify_each_bytes(ctx, h, buf, 1, 1, 3, xs, ok, st), "validate")
        refused(dll.ark355_verify_each_bytes(ctx, h, buf, 1, 1, -1, xs, ok, st), "validate")
        refused(dll.ark355_verify_each_bytes(ctx, h, buf, (1 << 32) // 3 + 1, 1, FULL, xs, ok, st), "count")
        assert dll.ark355_verify_each_bytes(ctx, h, None, 0, 1, FULL, None, None, None) == 0            # count = 0
        assert list(ok) == [7, 7, 7, 7] and list(st) == [9, 9, 9, 9]
        refused(dll.ark355_verify_each_bytes(ctx, h, buf, 1, 1, FULL, None, ok, st), "public_inputs")
        assert lib.verify_each_bytes(ctx, h, b"", 0, b"", True, FULL) == ([], [])
        # the handle still serves after the refusals, and a broken proof is an answer, not an error
        assert lib.verify_each_bytes(ctx, h, wire, 1, batch[2][0], True, FULL) == ([True], [0])
        assert lib.verify_each_bytes(ctx, h, bytes(len(wire)), 1, batch[2][0], True, FULL)[0] == [False]
    refused(dll.ark355_proofs_from_bytes(ctx, C.curve_id, None, 1, 1, FULL, out, st), "in")
    refused(dll.ark355_proofs_from_bytes(ctx, C.curve_id, buf, 1, 1, FULL, None, st), "out")
    refused(dll.ark355_proofs_from_bytes(ctx, C.curve_id, buf, 1, 1, FULL, out, None), "status")
    refused(dll.ark355_proofs_from_bytes(ctx, C.curve_id, buf, 1, 1, 7, out, st), "validate")
    refused(dll.ark355_proofs_from_bytes(ctx, C.curve_id, buf, (1 << 32) // 3 + 1, 1, FULL, out, st), "count")
    assert dll.ark355_proofs_from_bytes(ctx, 99, buf, 1, 1, FULL, out, st) == einval
    assert dll.ark355_proofs_from_bytes(ctx, C.curve_id, None, 0, 1, FULL, None, None) == 0
    assert dll.ark355_proofs_from_bytes(None, C.curve_id, buf, 1, 1, FULL, out, st) == einval
    refused(dll.ark355_points_check(ctx, C.curve_id, 1, None, 1, 1, st), "raw")
    refused(dll.ark355_points_check(ctx, C.curve_id, 1, raw, 1, 1, None), "status")
    refused(dll.ark355_points_check(ctx, C.curve_id, 1, raw, 1, 2, st), "method")
    refused(dll.ark355_points_check(ctx, C.curve_id, 3, raw, 1, 1, st), "group")
    assert dll.ark355_points_check(ctx, C.curve_id, 1, None, 0, 1, None) == 0
    assert list(st) == [9, 9, 9, 9]
    assert lib.points_check(ctx, C.curve_id, 1, batch[1][0][0], 1) == [0]


def groth16_case(lib, C):
    """snark_amd.Groth16.verify_each_bytes: the verdicts of verify_each on the decoded proofs, the statuses of the decoder; the
    key is processed on first use; a list of encoded proofs and one block of them are the same call."""
    from snark_amd.groth16 import Groth16, Proof, VerifyingKey
    batch, _, objs, inputs = oracle_proofs(C)
    parts, proofs = batch[0], batch[1]
    g = Groth16(C.name, lib=lib)
    try:
        vk = VerifyingKey(*parts)
        good = Z.proof_bytes(C, objs[0], True)
        other_c = Z.proof_bytes(C, G.Proof(objs[0].a, objs[0].b, objs[1].c), True)
        broken = split(C, good, True)
        broken[1] = damages(C, 2, True)[-3][1]
        wires = [good, other_c, b"".join(broken), good]
        xs = [inputs[0], inputs[0], inputs[0], inputs[0][:-1]]
        assert getattr(vk, "_ark355_pvk", None) is None
        oks, st = g.verify_each_bytes(vk, xs, wires)
        assert vk._ark355_pvk[0] is g                                       # processed on first use
        assert st == [0, 0, (2 << 4) | Z.NOT_IN_SUBGROUP, 0]
        decoded = [Proof(*proofs[0]), Proof(proofs[0][0], proofs[0][1], proofs[1][2])]
        assert oks[:2] == g.verify_each(vk, xs[:2], decoded) == [True, False]
        assert oks[2:] == [False, False]                                    # undecodable; wrong input length
        assert g.verify_each_bytes(vk, xs[:3], b"".join(wires[:3])) == (oks[:3], st[:3])
        assert g.verify_each_bytes(vk, xs[:3], b"".join(wires[:3]), validate=CURVE)[1] == [0, 0, 0]
        unc = [Z.proof_bytes(C, objs[0], False)]
        assert g.verify_each_bytes(vk, xs[:1], unc, compressed=False) == ([True], [0])
    finally:
        g.close()
