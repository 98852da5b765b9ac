"""Per-group pairing cases shared by the CPU-emulator tier (test_emul_pairing_each.py) and the GPU tier
(test_gpu_pairing_each.py): `ark355_pairing_groups` and `ark355_verify_each` through `snark_amd._binding.Lib`, against
oracle/pairing.py.

As in pairing_cases.py the pairs have known discrete logarithms, P_i = a_i G1 and Q_i = b_i G2, so the GT of a group is
e(G1, G2)^(sum over the group of a_i b_i): one power in GT per group on the oracle's side."""
from __future__ import annotations

import os
import random
import re

import pytest

from helpers import z_bytes
from oracle import serialize as Z
from pairing_cases import expected_gt, gt_to_flat, mixed_scalars, non_subgroup_g2, pairing_of, points_with_dlogs

GT_SHAPES = [(1, 1), (2, 1), (65, 1), (22, 3), (5, 4), (3, 64)]
PLANTED = (0, 21, 5461, 10921, 10922)


def group_scalars(C, groups, group_len, seed):
    """`groups` groups of mixed_scalars (infinities on either side included), then one group whose product is one (a pair and
    its negation; with group_len = 1 a pair with P at infinity) and one all-infinity group."""
    a, b = mixed_scalars(C, groups * group_len, seed)
    rnd = random.Random(seed + 1)
    s, t = rnd.randrange(1, C.r), rnd.randrange(1, C.r)
    if group_len >= 2:
        a += [s, C.r - s] + [0] * (group_len - 2)
        b += [t, t] + [0] * (group_len - 2)
    else:
        a += [0]
        b += [t]
    a += [0] * group_len
    b += [0] * group_len
    return a, b, groups + 2


def group_sums(C, a, b, group_len):
    return [sum(x * y for x, y in zip(a[k:k + group_len], b[k:k + group_len])) % C.r for k in range(0, len(a), group_len)]


def gt_groups_case(lib, ctx, C, groups, group_len, seed=71):
    """Every group's GT against e(G1, G2)^(sum a_i b_i); is_one exactly where the sum is 0 mod r, and both values occur."""
    sz = lib.sizes(C.curve_id)
    a, b, total = group_scalars(C, groups, group_len, seed)
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=1)
    gt, one = lib.pairing_groups(ctx, C.curve_id, p, q, total, group_len)
    sums = group_sums(C, a, b, group_len)
    assert len(sums) == total and len(gt) == total * 12 * sz["fq"]
    F = pairing_of(C).F
    for k, s in enumerate(sums):
        got = gt_to_flat(C, gt[k * 12 * sz["fq"]:(k + 1) * 12 * sz["fq"]])
        assert F.eq(got, expected_gt(C, s)), (C.name, groups, group_len, k)
    assert one == [s == 0 for s in sums]
    assert True in one and False in one
    # is_one alone, no GT
    none, one2 = lib.pairing_groups(ctx, C.curve_id, p, q, total, group_len, want_gt=False)
    assert none is None and one2 == one


def groups_match_multi_pairing_case(lib, ctx, C, groups, group_len, seed=73):
    """Every GT value is byte for byte what ark355_multi_pairing returns for that group's pairs alone."""
    sz = lib.sizes(C.curve_id)
    a, b, total = group_scalars(C, groups, group_len, seed)
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=0)
    gt, one = lib.pairing_groups(ctx, C.curve_id, p, q, total, group_len)
    w = 12 * sz["fq"]
    for k in range(total):
        lo, hi = k * group_len, (k + 1) * group_len
        g, o = lib.multi_pairing(ctx, C.curve_id, p[lo * sz["g1"]:hi * sz["g1"]], q[lo * sz["g2"]:hi * sz["g2"]], group_len)
        assert g == gt[k * w:(k + 1) * w] and o == one[k], (C.name, k)


def routes_agree_each_case(lib, ctx, policy, C, groups, group_len, seed=79):
    """PAIRING_DEVICE=0 (host threads, PairingHost::final_exponentiation per group) and =1 (device) give byte-equal GT."""
    a, b, total = group_scalars(C, groups, group_len, seed)
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=1)
    policy.setenv("ARK355_PAIRING_DEVICE", 0)
    host = lib.pairing_groups(ctx, C.curve_id, p, q, total, group_len)
    policy.setenv("ARK355_PAIRING_DEVICE", 1)
    dev = lib.pairing_groups(ctx, C.curve_id, p, q, total, group_len)
    assert host == dev, (C.name, groups, group_len)
    assert any(host[0]) and True in host[1] and False in host[1]


def chunk_case(lib, ctx, C, groups=10923, planted=PLANTED, seed=83):
    """Past the 2^15-pair chunk: groups of (a G1, b G2), (-a G1, b G2), infinity; at the planted groups the third pair is
    (c G1, G2).  is_one everywhere but there, every other GT the image of one, the planted ones e(G1, G2)^c."""
    sz = lib.sizes(C.curve_id)
    rnd = random.Random(seed)
    a, b, cs = [], [], {}
    for k in range(groups):
        s, t = rnd.randrange(1, C.r), rnd.randrange(1, C.r)
        a += [s, C.r - s, 0]
        b += [t, t, 0]
        if k in planted:
            cs[k] = rnd.randrange(1, C.r)
            a[-1], b[-1] = cs[k], 1
    assert 3 * groups > 1 << 15 and len(cs) == len(planted)
    p, q = points_with_dlogs(lib, ctx, C, a, b)
    gt, one = lib.pairing_groups(ctx, C.curve_id, p, q, groups, 3)
    assert one == [k not in cs for k in range(groups)]
    F = pairing_of(C).F
    w = 12 * sz["fq"]
    unit = gt[w:2 * w]                                  # group 1 is not planted
    assert F.eq(gt_to_flat(C, unit), F.one)
    for k in range(groups):
        if k in cs:
            assert F.eq(gt_to_flat(C, gt[k * w:(k + 1) * w]), expected_gt(C, cs[k])), (C.name, k)
        else:
            assert gt[k * w:(k + 1) * w] == unit, (C.name, k)


def refusals_each_case(lib, ctx, C, err_type, einval, groups=3, group_len=2):
    """Off-curve points at a middle index are refused by name (index into the flat list), group_len 0 and 65 are refused with
    a pointer to ark355_multi_pairing, groups = 0 is accepted, a NULL array with pairs to read is refused, a point of the twist
    outside the subgroup returns cleanly."""
    sz = lib.sizes(C.curve_id)
    n = groups * group_len
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
            lib.pairing_groups(ctx, C.curve_id, pp, qq, groups, group_len)
        assert e.value.code == einval and "%s[%d]" % (which, mid) in str(e.value), str(e.value)
    for bad_len in (0, 65):
        with pytest.raises(err_type) as e:
            lib.pairing_groups(ctx, C.curve_id, p, q, 1, bad_len)
        assert e.value.code == einval and "ark355_multi_pairing" in str(e.value), str(e.value)
    gt, one = lib.pairing_groups(ctx, C.curve_id, b"", b"", 0, group_len)
    assert gt == b"" and one == []
    with pytest.raises(err_type) as e:
        lib.pairing_groups(ctx, C.curve_id, b"", q, groups, group_len)
    assert e.value.code == einval
    X = non_subgroup_g2(C)
    qq = bytearray(q)
    qq[mid * sz["g2"]:(mid + 1) * sz["g2"]] = Z.g2_raw(C, X)
    gt, one = lib.pairing_groups(ctx, C.curve_id, p, bytes(qq), groups, group_len)
    assert len(gt) == groups * 12 * sz["fq"] and len(one) == groups


def _wrong_input(C, zs, ell, j, k):
    z = zs[j % k]
    return z_bytes(C, [(z[1] + 1) % C.r] + list(z[2:ell]))


def tampered_batch(C, batch, total, other_c=(), wrong_input=(), a_inf=(), b_off=(), swapped=()):
    """`total` proofs cycling the oracle-made ones, tampered at the given indices -> (proofs, inputs, expected verdicts)."""
    vk, proofs, inputs, zs, ell = batch
    k = len(proofs)
    ps = [proofs[j % k] for j in range(total)]
    xs = [inputs[j % k] for j in range(total)]
    ok = [True] * total
    for j in other_c:                                   # C of another proof
        ps[j] = (ps[j][0], ps[j][1], proofs[(j + 1) % k][2])
    for j in wrong_input:                               # one public input off by one
        xs[j] = _wrong_input(C, zs, ell, j, k)
    for j in a_inf:                                     # A at infinity
        ps[j] = (bytes(len(ps[j][0])), ps[j][1], ps[j][2])
    for j in b_off:                                     # one byte of B poked off the curve
        raw = bytearray(ps[j][1])
        raw[len(raw) // 2] ^= 1
        ps[j] = (ps[j][0], bytes(raw), ps[j][2])
    for j in swapped:                                   # A and B of one proof with C of another
        o = proofs[(j + 3) % k]
        ps[j] = (o[0], o[1], ps[j][2])
    for j in list(other_c) + list(wrong_input) + list(a_inf) + list(b_off) + list(swapped):
        ok[j] = False
    return ps, xs, ok


def verify_each_case(lib, ctx, policy, C, batch, err_type, einval, total=130, tamper=None, singles=(1, 66, 128)):
    """The verdict list is exact on both routes; for the tampered indices and a few good ones ok[j] equals ark355_verify_batch
    of that proof alone; a key with gamma_g2 poked off its curve is the caller's error."""
    if tamper is None:
        tamper = dict(other_c=(0,), wrong_input=(63,), a_inf=(64,), b_off=(65,), swapped=(129,))
    vk = batch[0]
    ps, xs, want = tampered_batch(C, batch, total, **tamper)
    got = {}
    for route in (1, 0):
        policy.setenv("ARK355_PAIRING_DEVICE", route)
        got[route] = lib.verify_each(ctx, C.curve_id, vk, ps, b"".join(xs))
        assert got[route] == want, (C.name, route, [j for j in range(total) if got[route][j] != want[j]])
    policy.setenv("ARK355_PAIRING_DEVICE", 1)
    for j in [i for v in tamper.values() for i in v] + [s for s in singles if s < total]:
        assert lib.verify_batch(ctx, C.curve_id, vk, [ps[j]], xs[j], None) == want[j], (C.name, j)
    bad = bytearray(vk[2])
    bad[len(bad) // 2] ^= 1
    with pytest.raises(err_type) as e:
        lib.verify_each(ctx, C.curve_id, (vk[0], vk[1], bytes(bad), vk[3], vk[4]), ps[:2], b"".join(xs[:2]))
    assert e.value.code == einval and "gamma_g2" in str(e.value), str(e.value)


def verify_each_default_policy_case(lib, ctx, policy, C, batch, total=4096, tamper=(0, 2047, 4000, 4095)):
    """Default policy (-1): `total` proofs are above PAIRING_EACH_MIN; the list is exact."""
    policy.setenv("ARK355_PAIRING_DEVICE", -1)
    assert lib.ctx_get_policy(ctx, "PAIRING_EACH_MIN") < total
    ps, xs, want = tampered_batch(C, batch, total, other_c=tamper[:2], wrong_input=tamper[2:3], swapped=tamper[3:])
    assert lib.verify_each(ctx, C.curve_id, batch[0], ps, b"".join(xs)) == want
    assert want.count(False) == len(tamper)


def no_public_inputs_case(lib, ctx, C):
    """num_instance == 1: acc = gamma_abc_0, public_inputs NULL.  With alpha = a G1, beta = b G2, gamma = delta = G2,
    gamma_abc_0 = s G1, the proof (A, B, C) = (x G1, y G2, z G1) verifies iff x y = a b + s + z mod r."""
    rnd = random.Random(89)
    a, b, s, x, y = (rnd.randrange(1, C.r) for _ in range(5))
    z = (x * y - a * b - s) % C.r
    g1s, g2s = points_with_dlogs(lib, ctx, C, [a, s, x, z, (z + 1) % C.r], [b, 1, y, 1, 1], cross_check=1)
    n1, n2 = lib.sizes(C.curve_id)["g1"], lib.sizes(C.curve_id)["g2"]
    P = [g1s[i * n1:(i + 1) * n1] for i in range(5)]
    Q = [g2s[i * n2:(i + 1) * n2] for i in range(5)]
    vk = (P[0], Q[0], Q[1], Q[1], P[1])
    assert lib.verify_each(ctx, C.curve_id, vk, [(P[2], Q[2], P[3]), (P[2], Q[2], P[4])], b"") == [True, False]


def default_each_route_case(lib, root):
    """A fresh context (the session's may carry another test's policy): PAIRING_DEVICE = -1 and the crossover DESIGN.md
    states as `PAIRING_EACH_MIN` = <value>."""
    names = ("ARK355_PAIRING_DEVICE", "ARK355_PAIRING_EACH_MIN")
    env = {k: os.environ.pop(k) for k in names if k in os.environ}
    try:
        ctx = lib.ctx_create(0)
    finally:
        os.environ.update(env)
    try:
        assert lib.ctx_get_policy(ctx, "PAIRING_DEVICE") == -1
        m = re.search(r"`PAIRING_EACH_MIN` = (\d+)", open(os.path.join(root, "DESIGN.md")).read())
        assert m, "DESIGN.md must state the crossover as `PAIRING_EACH_MIN` = <value>"
        assert lib.ctx_get_policy(ctx, "PAIRING_EACH_MIN") == int(m.group(1))
    finally:
        lib.ctx_destroy(ctx)
