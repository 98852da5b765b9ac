"""Cases that hold the four entries of snark_amd/csrc/verify_impl.cuh (`ark355_multi_pairing`, `ark355_pairing_groups`,
`ark355_verify_each`, `ark355_verify_batch`) to what their two routes share: the TRACE_HOST phase lines, the verdict of
`ark355_verify_batch`, and the texts a point off its curve is refused with.  Drivers: test_emul_verify.py (CPU emulator) and
test_gpu_verify.py (MI355X)."""
from __future__ import annotations

import os
import random
import sys

import pytest

from conftest import ROOT
from helpers import z_bytes
from oracle import serialize as Z
from pairing_cases import mixed_scalars, points_with_dlogs

ROUTES = {0: "host", 1: "device"}


def phase_regex():
    """the expression tools/pairing_bench.py reads the phase lines with"""
    tools = os.path.join(ROOT, "tools")
    sys.path.insert(0, tools)
    try:
        from pairing_bench import PHASE
    finally:
        sys.path.remove(tools)
    return PHASE


def poke(raw: bytes, size: int, idx: int = 0) -> bytes:
    """point `idx` of an array of `size`-byte raw images with the lowest byte of y (of y.c0 in G2) flipped: still reduced, no
    longer on the curve"""
    out = bytearray(raw)
    out[idx * size + size // 2] ^= 1
    return bytes(out)


def trace_case(lib, ctx, policy, capfd, C, batch):
    """Under TRACE_HOST every entry writes one phase line per call on either route, in the form pairing_bench.py parses:
    its own name, the route taken, and the pairs it ran (n, count + 3, groups * group_len, 3 * count).  The host route of
    verify_batch stops after scalar_mul_ms; every other line carries all four phases."""
    PHASE = phase_regex()
    sz = lib.sizes(C.curve_id)
    vk, proofs, inputs = batch[0], batch[1][:2], b"".join(batch[2][:2])
    a, b = mixed_scalars(C, 4, seed=97)
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=0)
    rho = [Z.fr_canon(C, 3), Z.fr_canon(C, 5)]
    calls = [
        ("multi_pairing", 2, lambda: lib.multi_pairing(ctx, C.curve_id, p[:2 * sz["g1"]], q[:2 * sz["g2"]], 2)),
        ("verify_batch", 2 + 3, lambda: lib.verify_batch(ctx, C.curve_id, vk, proofs, inputs, rho)),
        ("pairing_groups", 2 * 2, lambda: lib.pairing_groups(ctx, C.curve_id, p, q, 2, 2)),
        ("verify_each", 3 * 2, lambda: lib.verify_each(ctx, C.curve_id, vk, proofs, inputs)),
    ]
    policy.setenv("ARK355_TRACE_HOST", 1)
    for route, route_name in ROUTES.items():
        policy.setenv("ARK355_PAIRING_DEVICE", route)
        for what, pairs, call in calls:
            capfd.readouterr()
            call()
            err = capfd.readouterr().err
            found = [m for m in map(PHASE.search, err.splitlines()) if m and m.group(1) == what]
            assert len(found) == 1, (what, route_name, err)
            m = found[0]
            assert m.string == m.group(0), m.string                      # nothing before or after what the expression reads
            assert (m.group(2), int(m.group(3))) == (route_name, pairs), m.string
            short = what == "verify_batch" and route == 0
            assert (m.group(6) is None) == short and (m.group(7) is None) == short, m.string


def verify_batch_routes_case(lib, ctx, policy, C, batch, count):
    """ark355_verify_batch of `count` proofs (the oracle-made ones cycled, distinct rho; rho = NULL for one proof) gives the same
    verdict under PAIRING_DEVICE = 0 and = 1: true for the valid batch; false with the last proof's C replaced, with one public
    input off by one, with a proof set against the next statement, and -- without raising -- with an A off its curve."""
    vk, proofs, inputs, zs, ell = batch
    k = len(proofs)
    assert k >= 2
    rnd = random.Random(101 + count)
    ps = [proofs[j % k] for j in range(count)]
    xs = [inputs[j % k] for j in range(count)]
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(count)] if count > 1 else None
    last, mid = count - 1, count // 2
    tampered = list(ps)
    tampered[last] = (ps[last][0], ps[last][1], proofs[(last + 1) % k][2])
    wrong = list(xs)
    z = zs[mid % k]
    wrong[mid] = z_bytes(C, [(z[1] + 1) % C.r] + list(z[2:ell]))
    other = list(ps)
    other[mid] = proofs[(mid + 1) % k]
    off = list(ps)
    off[mid] = (poke(ps[mid][0], len(ps[mid][0])), ps[mid][1], ps[mid][2])
    cases = [("valid", ps, xs, True), ("tampered proof", tampered, xs, False), ("wrong public input", ps, wrong, False),
             ("proof of another statement", other, xs, False), ("A off the curve", off, xs, False)]
    for name, pp, xx, want in cases:
        got = {}
        for route in ROUTES:
            policy.setenv("ARK355_PAIRING_DEVICE", route)
            got[route] = lib.verify_batch(ctx, C.curve_id, vk, pp, b"".join(xx), rho)
        assert got[0] == got[1] == want, (C.name, count, name, got)


def refusal_texts_case(lib, ctx, policy, C, batch, err_type, einval, n=5):
    """The texts a point off its curve is refused with, on both routes: `g1[i]` / `g2[i]` (index into the flat list) from
    multi_pairing and pairing_groups over n pairs, `vk.alpha_g1` and `vk.gamma_abc_g1[i]` from verify_each."""
    sz = lib.sizes(C.curve_id)
    a, b = mixed_scalars(C, n, seed=59)
    a[1], b[2] = 7, 9
    p, q = points_with_dlogs(lib, ctx, C, a, b, cross_check=0)
    mid = n // 2
    vk, proofs, inputs = batch[0], batch[1][:2], b"".join(batch[2][:2])
    i = len(vk[4]) // sz["g1"] - 1
    assert i >= 1
    bad_alpha = (poke(vk[0], sz["g1"]),) + tuple(vk[1:])
    bad_abc = tuple(vk[:4]) + (poke(vk[4], sz["g1"], i),)
    calls = [
        ("g1[%d]" % mid, lambda: lib.multi_pairing(ctx, C.curve_id, poke(p, sz["g1"], mid), q, n)),
        ("g2[%d]" % mid, lambda: lib.multi_pairing(ctx, C.curve_id, p, poke(q, sz["g2"], mid), n)),
        ("g1[%d]" % mid, lambda: lib.pairing_groups(ctx, C.curve_id, poke(p, sz["g1"], mid), q, n, 1)),
        ("g2[%d]" % mid, lambda: lib.pairing_groups(ctx, C.curve_id, p, poke(q, sz["g2"], mid), n, 1)),
        ("vk.alpha_g1", lambda: lib.verify_each(ctx, C.curve_id, bad_alpha, proofs, inputs)),
        ("vk.gamma_abc_g1[%d]" % i, lambda: lib.verify_each(ctx, C.curve_id, bad_abc, proofs, inputs)),
    ]
    for route in ROUTES:
        policy.setenv("ARK355_PAIRING_DEVICE", route)
        for where, call in calls:
            with pytest.raises(err_type) as e:
                call()
            assert e.value.code == einval
            assert str(e.value).split(": ", 1)[1] == where + ": point not on curve", (route, str(e.value))
