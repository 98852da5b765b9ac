"""Processed-verifying-key cases shared by the CPU-emulator tier (test_emul_pvk.py) and the GPU tier (test_gpu_pvk.py):
`ark355_vk_process` and the entries that take its handle, through `snark_amd._binding.Lib`.

The yardsticks are the entries that take the bare key: `ark355_pvk_pairings` must give the bytes of `ark355_pairing_groups`
(the Miller value through shared lines is bit-identical to the one through per-pair lines), `ark355_verify_each_pvk` the
verdicts of `ark355_verify_each`, `ark355_verify_batch_pvk` the verdict of `ark355_verify_batch`."""
from __future__ import annotations

import contextlib
import ctypes
import os
import random
import re

import pytest

from conftest import ROOT
from oracle import serialize as Z
from pairing_cases import expected_gt, gt_to_flat, non_subgroup_g2, pairing_of, points_with_dlogs
from pairing_each_cases import tampered_batch

WHICH = {0: 1, 1: 2, 2: 3}          # which -> index of the point in the vk parts (alpha, beta, gamma, delta, gamma_abc)


@contextlib.contextmanager
def processed(lib, ctx, C, vk):
    h = lib.vk_process(ctx, C.curve_id, vk)
    try:
        yield h
    finally:
        lib.pvk_free(h)


def dlog_key(lib, ctx, C, seed=97, delta_inf=False, extra_g1=()):
    """A key with known discrete logarithms: alpha = a G1, (beta, gamma, delta) = b_i G2, gamma_abc = [s G1].
    -> (vk parts, dict of the scalars, the extra G1 points asked for)."""
    rnd = random.Random(seed)
    a, s = rnd.randrange(1, C.r), rnd.randrange(1, C.r)
    b = [rnd.randrange(1, C.r) for _ in range(3)]
    if delta_inf:
        b[2] = 0
    g1_scalars = [a, s] + list(extra_g1)
    n = max(len(g1_scalars), 3)
    p, q = points_with_dlogs(lib, ctx, C, g1_scalars + [1] * (n - len(g1_scalars)), b + [1] * (n - 3), cross_check=1)
    n1, n2 = lib.sizes(C.curve_id)["g1"], lib.sizes(C.curve_id)["g2"]
    P = [p[i * n1:(i + 1) * n1] for i in range(len(g1_scalars))]
    Q = [q[i * n2:(i + 1) * n2] for i in range(3)]
    return (P[0], Q[0], Q[1], Q[2], P[1]), dict(alpha=a, beta=b[0], gamma=b[1], delta=b[2], abc0=s), P[2:]


def g1_points(lib, ctx, C, n, seed, inf=()):
    rnd = random.Random(seed * 31 + n)
    a = [0 if i in inf else rnd.randrange(1, C.r) for i in range(n)]
    p, _ = points_with_dlogs(lib, ctx, C, a, [1] * n, cross_check=1)
    return a, p


def pairings_match_groups_case(lib, ctx, C, n, whiches=(0, 1, 2), inf=(), seed=101):
    """e(P_i, Q_which) from the handle, byte for byte what ark355_pairing_groups gives for (P_i, Q) pairs; is_one at the
    points at infinity and nowhere else; is_one alone without GT."""
    vk, _, _ = dlog_key(lib, ctx, C)
    _, p = g1_points(lib, ctx, C, n, seed, inf)
    with processed(lib, ctx, C, vk) as h:
        for which in whiches:
            want = lib.pairing_groups(ctx, C.curve_id, p, vk[WHICH[which]] * n, n, 1)
            got = lib.pvk_pairings(ctx, h, which, p, n)
            assert got == want, (C.name, n, which)
            assert got[1] == [i in inf for i in range(n)]
            none, one = lib.pvk_pairings(ctx, h, which, p, n, want_gt=False)
            assert none is None and one == want[1]


def pairings_oracle_case(lib, ctx, C, n=5, seed=103):
    """Against the oracle: e(a_i G1, b G2) = e(G1, G2)^(a_i b)."""
    vk, k, _ = dlog_key(lib, ctx, C)
    a, p = g1_points(lib, ctx, C, n, seed)
    F = pairing_of(C).F
    w = 12 * lib.sizes(C.curve_id)["fq"]
    with processed(lib, ctx, C, vk) as h:
        for which, name in ((0, "beta"), (1, "gamma"), (2, "delta")):
            gt, one = lib.pvk_pairings(ctx, h, which, p, n)
            for i in range(n):
                assert F.eq(gt_to_flat(C, gt[i * w:(i + 1) * w]), expected_gt(C, a[i] * k[name])), (C.name, name, i)
            assert one == [False] * n


def delta_at_infinity_pairings_case(lib, ctx, C, n=3):
    """A key whose delta is the point at infinity is legal: every pairing against it is one."""
    vk, _, _ = dlog_key(lib, ctx, C, delta_inf=True)
    assert vk[3] == bytes(len(vk[3]))
    _, p = g1_points(lib, ctx, C, n, seed=107)
    with processed(lib, ctx, C, vk) as h:
        gt, one = lib.pvk_pairings(ctx, h, 2, p, n)
        assert one == [True] * n
        assert (gt, one) == lib.pairing_groups(ctx, C.curve_id, p, vk[3] * n, n, 1)
        assert lib.pvk_pairings(ctx, h, 1, p, n)[1] == [False] * n


def alpha_beta_case(lib, ctx, C, vk):
    """alpha_g1_beta_g2 of the handle is ark355_multi_pairing's value for the one pair, and the handle describes its key."""
    sz = lib.sizes(C.curve_id)
    with processed(lib, ctx, C, vk) as h:
        assert lib.pvk_alpha_beta(h) == lib.multi_pairing(ctx, C.curve_id, vk[0], vk[1], 1)[0]
        info = lib.pvk_info(h)
        assert info["curve"] == C.curve_id and info["num_instance"] == len(vk[4]) // sz["g1"]
        assert info["resident_bytes"] > len(vk[4])
        assert lib.dll.ark355_pvk_info(h, None, None, None) == 0


def verify_each_pvk_case(lib, ctx, policy, C, batch, total=130, tamper=None):
    """The verdict list is exact on both routes, equals ark355_verify_each's, and at the tampered indices
    ark355_verify_batch_pvk of that proof alone."""
    if tamper is None:
        tamper = dict(other_c=(0,), wrong_input=(63,), a_inf=(64,), b_off=(65,), swapped=(129,))
    vk = batch[0]
    ps, xs, want = tampered_batch(C, batch, total, **tamper)
    with processed(lib, ctx, C, vk) as h:
        for route in (1, 0):
            policy.setenv("ARK355_PAIRING_DEVICE", route)
            got = lib.verify_each_pvk(ctx, h, ps, b"".join(xs))
            assert got == want, (C.name, route, [j for j in range(total) if got[j] != want[j]])
            assert got == lib.verify_each(ctx, C.curve_id, vk, ps, b"".join(xs)), (C.name, route)
        policy.setenv("ARK355_PAIRING_DEVICE", 1)
        for j in [i for v in tamper.values() for i in v]:
            assert lib.verify_batch_pvk(ctx, h, [ps[j]], xs[j], None) == want[j], (C.name, j)


def verify_each_pvk_default_policy_case(lib, ctx, policy, C, batch, total=4096, tamper=(0, 2047, 4000, 4095)):
    """Default policy (-1): `total` proofs are above PAIRING_EACH_MIN; the list is exact."""
    policy.setenv("ARK355_PAIRING_DEVICE", -1)
    assert lib.ctx_get_policy(ctx, "PAIRING_EACH_MIN") < total
    ps, xs, want = tampered_batch(C, batch, total, other_c=tamper[:2], wrong_input=tamper[2:3], swapped=tamper[3:])
    with processed(lib, ctx, C, batch[0]) as h:
        assert lib.verify_each_pvk(ctx, h, ps, b"".join(xs)) == want
    assert want.count(False) == len(tamper)


def each_chunk_proofs():
    """Proofs a chunk of ark355_verify_each_pvk holds, read from the constants next to PAIR_CHUNK in verify_impl.cuh."""
    src = open(os.path.join(ROOT, "snark_amd", "csrc", "verify_impl.cuh")).read()
    pair = re.search(r"PAIR_CHUNK = 1u << (\d+);", src)
    each = re.search(r"PVK_EACH_CHUNK = ([^;]+);", src)
    assert pair and each, "verify_impl.cuh must state PAIR_CHUNK and PVK_EACH_CHUNK"
    pair_chunk = 1 << int(pair.group(1))
    expr = each.group(1).strip()
    if expr == "PAIR_CHUNK":
        return pair_chunk
    assert expr == "PAIR_CHUNK / 3", expr
    return pair_chunk // 3


def past_the_chunk_case(lib, ctx, C, batch, total):
    """`total` proofs with a planted failure in the first and the last proof of every chunk."""
    chunk = each_chunk_proofs()
    planted = sorted({j for c in range(0, total, chunk) for j in (c, min(c + chunk, total) - 1)})
    ps, xs, want = tampered_batch(C, batch, total, other_c=planted)
    with processed(lib, ctx, C, batch[0]) as h:
        got = lib.verify_each_pvk(ctx, h, ps, b"".join(xs))
    assert got == want, (C.name, total, [j for j in range(total) if got[j] != want[j]][:8])
    assert want.count(False) == len(planted)


def no_public_inputs_case(lib, ctx, C, delta_inf=False):
    """num_instance == 1 (the construction of pairing_each_cases.no_public_inputs_case): gamma = G2 and delta = G2, or delta at
    infinity, where the equation becomes x y = a b + s.  The plain entry is the reference either way."""
    rnd = random.Random(89)
    a, b, s, x, y = (rnd.randrange(1, C.r) for _ in range(5))
    z = (x * y - a * b - s) % C.r
    if delta_inf:
        s = (x * y - a * b) % C.r
    g1s, g2s = points_with_dlogs(lib, ctx, C, [a, s, x, z, (z + 1) % C.r, (s + 1) % C.r], [b, 1, y, 0, 1, 1], cross_check=1)
    n1, n2 = lib.sizes(C.curve_id)["g1"], lib.sizes(C.curve_id)["g2"]
    P = [g1s[i * n1:(i + 1) * n1] for i in range(6)]
    Q = [g2s[i * n2:(i + 1) * n2] for i in range(6)]
    vk = (P[0], Q[0], Q[1], Q[3] if delta_inf else Q[1], P[1])
    proofs = [(P[2], Q[2], P[3]), (P[2], Q[2], P[4])]
    want = [True, True] if delta_inf else [True, False]        # C pairs with the point at infinity: it no longer matters
    with processed(lib, ctx, C, vk) as h:
        assert lib.verify_each_pvk(ctx, h, proofs, b"") == want == lib.verify_each(ctx, C.curve_id, vk, proofs, b"")
    if delta_inf:                                              # and a key that states another s rejects both
        bad = vk[:4] + (P[5],)
        with processed(lib, ctx, C, bad) as h:
            assert lib.verify_each_pvk(ctx, h, proofs, b"") == [False, False] == lib.verify_each(ctx, C.curve_id, bad, proofs, b"")


def non_subgroup_gamma_case(lib, ctx, C, batch):
    """A gamma on the twist outside the subgroup returns cleanly, as the plain entry does (whatever the verdicts)."""
    vk, proofs, inputs = batch[0], batch[1], batch[2]
    odd = (vk[0], vk[1], Z.g2_raw(C, non_subgroup_g2(C)), vk[3], vk[4])
    with processed(lib, ctx, C, odd) as h:
        got = lib.verify_each_pvk(ctx, h, proofs[:2], b"".join(inputs[:2]))
    assert len(got) == 2
    assert len(lib.verify_each(ctx, C.curve_id, odd, proofs[:2], b"".join(inputs[:2]))) == 2


def verify_batch_pvk_case(lib, ctx, C, batch, count=5):
    """count = 1 with rho = NULL; `count` proofs with 128-bit rho, good and with one tampered proof: each the verdict of
    ark355_verify_batch."""
    vk, proofs, inputs = batch[0], batch[1], batch[2]
    k = len(proofs)
    rnd = random.Random(109)
    ps = [proofs[j % k] for j in range(count)]
    xs = b"".join(inputs[j % k] for j in range(count))
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(count)]
    with processed(lib, ctx, C, vk) as h:
        assert lib.verify_batch_pvk(ctx, h, ps[:1], inputs[0], None) is True
        assert lib.verify_batch(ctx, C.curve_id, vk, ps[:1], inputs[0], None) is True
        if count > 1:
            bad = list(ps)
            bad[count // 2] = (ps[count // 2][0], ps[count // 2][1], proofs[(count // 2 + 1) % k][2])
            for cand, want in ((ps, True), (bad, False)):
                assert lib.verify_batch_pvk(ctx, h, cand, xs, rho) is want
                assert lib.verify_batch(ctx, C.curve_id, vk, cand, xs, rho) is want
        else:
            other = (ps[0][0], ps[0][1], proofs[1 % k][2])
            assert lib.verify_batch_pvk(ctx, h, [other], inputs[0], None) is False


def sharing_case(lib, ctx, C, batch, total=3):
    """A handle made through one context gives the same verdicts from a second one, and keeps working after the context that
    made it is destroyed: the handle belongs to the device, not to the context (include/ark355.h)."""
    ps, xs, want = tampered_batch(C, batch, total, other_c=(1,))
    maker = lib.ctx_create(0)
    try:
        h = lib.vk_process(maker, C.curve_id, batch[0])
        try:
            assert lib.verify_each_pvk(maker, h, ps, b"".join(xs)) == want
            assert lib.verify_each_pvk(ctx, h, ps, b"".join(xs)) == want
        except BaseException:
            lib.pvk_free(h)
            raise
    finally:
        lib.ctx_destroy(maker)
    try:
        assert lib.verify_each_pvk(ctx, h, ps, b"".join(xs)) == want
        assert lib.pvk_alpha_beta(h) == lib.multi_pairing(ctx, C.curve_id, batch[0][0], batch[0][1], 1)[0]
    finally:
        lib.pvk_free(h)


def refusals_case(lib, ctx, C, batch, err_type, einval):
    """A key point off its curve is refused by name at process time; NULL arguments, which = 3 and a NULL g1 with n > 0 are
    ARK355_EINVAL; a G1 argument off its curve is named with its index; count = 0 and n = 0 return OK and write nothing."""
    vk, proofs, inputs = batch[0], batch[1], batch[2]
    sz = lib.sizes(C.curve_id)

    def poke(buf, size, idx):
        raw = bytearray(buf)
        raw[idx * size + size // 2] ^= 1
        return bytes(raw)

    for name, bad in (("vk.gamma_g2", (vk[0], vk[1], poke(vk[2], sz["g2"], 0), vk[3], vk[4])),
                      ("vk.gamma_abc_g1[1]", (vk[0], vk[1], vk[2], vk[3], poke(vk[4], sz["g1"], 1)))):
        with pytest.raises(err_type) as e:
            lib.vk_process(ctx, C.curve_id, bad)
        assert e.value.code == einval and name in str(e.value) and "not on curve" in str(e.value), str(e.value)
    keep = []
    desc = lib._vk_desc(vk, keep)
    out = ctypes.c_void_p()
    dll = lib.dll
    assert dll.ark355_vk_process(ctx, C.curve_id, ctypes.byref(desc), None) == einval              # NULL out
    assert dll.ark355_vk_process(ctx, C.curve_id, None, ctypes.byref(out)) == einval and not out.value
    empty = lib._vk_desc(vk, keep)
    empty.num_instance = 0
    assert dll.ark355_vk_process(ctx, C.curve_id, ctypes.byref(empty), ctypes.byref(out)) == einval and not out.value
    assert dll.ark355_pvk_info(None, None, None, None) == einval                                    # NULL pvk
    gt = (ctypes.c_uint8 * (12 * sz["fq"]))()
    ok = (ctypes.c_uint8 * 4)(7, 7, 7, 7)
    verdict = ctypes.c_int32(7)
    assert dll.ark355_pvk_alpha_beta(None, gt) == einval
    assert dll.ark355_pvk_pairings(ctx, None, 0, vk[0], 1, None, None) == einval
    assert dll.ark355_verify_each_pvk(ctx, None, None, None, 0, None) == einval
    assert dll.ark355_verify_batch_pvk(ctx, None, None, None, None, 1, ctypes.byref(verdict)) == einval
    dll.ark355_pvk_free(None)
    with processed(lib, ctx, C, vk) as h:
        with pytest.raises(err_type) as e:
            lib.pvk_pairings(ctx, h, 3, vk[0], 1)
        assert e.value.code == einval and "which" in str(e.value)
        assert dll.ark355_pvk_pairings(ctx, h, 0, None, 2, None, None) == einval                  # NULL g1 with n > 0
        p = vk[4][:2 * sz["g1"]] + vk[0]
        with pytest.raises(err_type) as e:
            lib.pvk_pairings(ctx, h, 1, poke(p, sz["g1"], 1), 3)
        assert e.value.code == einval and "g1[1]" in str(e.value), str(e.value)
        assert lib.pvk_pairings(ctx, h, 1, b"", 0) == (b"", [])
        assert dll.ark355_verify_each_pvk(ctx, h, None, None, 0, ok) == 0 and list(ok) == [7, 7, 7, 7]   # count = 0
        assert lib.verify_each_pvk(ctx, h, [], b"") == []
        assert dll.ark355_verify_each_pvk(ctx, h, None, None, 1, ok) == einval                    # NULL proofs with count > 0
        assert dll.ark355_pvk_alpha_beta(h, None) == einval
        # the handle still serves after the refusals
        assert lib.verify_each_pvk(ctx, h, proofs[:1], inputs[0]) == [True]


def groth16_mirror_case(lib, C, batch):
    """snark_amd.Groth16 over `lib`: process_vk returns the key it was given with the handle attached, and
    verify_with_processed_vk / verify_each / verify_batch / alpha_g1_beta_g2 run against it."""
    from snark_amd.groth16 import Groth16, Proof, VerifyingKey
    parts, proofs, _, zs, ell = batch
    g = Groth16(C.name, lib=lib)
    try:
        vk = VerifyingKey(*parts)
        plain = g.alpha_g1_beta_g2(vk)
        assert getattr(vk, "_ark355_pvk", None) is None
        assert g.process_vk(vk) is vk and vk._ark355_pvk[0] is g
        handle = vk._ark355_pvk[1]
        assert g.process_vk(vk) is vk and vk._ark355_pvk[1] is handle          # processed once
        assert g.alpha_g1_beta_g2(vk) == plain
        good = Proof(*proofs[0])
        bad = Proof(proofs[0][0], proofs[0][1], proofs[1][2])
        x0 = list(zs[0][1:ell])
        assert g.verify_with_processed_vk(vk, x0, good) is True
        assert g.verify_with_processed_vk(vk, x0, bad) is False
        assert g.verify_with_processed_vk(vk, x0[:-1], good) is False          # wrong input length
        assert g.verify_each(vk, [x0, x0], [good, bad]) == [True, False]
        assert g.verify(vk, x0, good) is True and g.verify(vk, x0, bad) is False
        fresh = VerifyingKey(*parts)                                            # not processed yet: processed on first use
        assert g.verify_with_processed_vk(fresh, x0, good) is True and fresh._ark355_pvk[0] is g
    finally:
        g.close()
