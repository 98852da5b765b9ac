"""Device pairing behind the C ABI on the CPU emulator build (see tests/pairing_cases.py): the kernels of
snark_amd/csrc/pairing_impl.cuh compiled with g++ against the HIP emulator, at sizes a single host thread handles."""
import os
import re

import pytest

import pairing_cases as P
import parity_cases as pc
from conftest import ROOT
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error


@pytest.fixture
def device_route(emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return emul_policy


@pytest.mark.parametrize("C,n", [(BLS12_381, 1), (BLS12_381, 2), (BLS12_381, 4), (BN254, 3)],
                         ids=["bls-1", "bls-2", "bls-4", "bn-3"])
def test_gt_against_the_oracle(emul_lib, emul_ctx, device_route, C, n):
    P.gt_case(emul_lib, emul_ctx, C, n)


def test_gt_with_points_at_infinity(emul_lib, emul_ctx, device_route):
    """P at infinity, Q at infinity, both: each contributes one."""
    C = BLS12_381
    a, b = [5, 0, 7, 0], [C.r - 1, 3, 0, 0]
    pts = (a, b) + P.points_with_dlogs(emul_lib, emul_ctx, C, a, b)
    P.gt_case(emul_lib, emul_ctx, C, 4, points=pts)


@pytest.mark.parametrize("C,n", [(BLS12_381, 3), (BN254, 2)], ids=["bls-3", "bn-2"])
def test_routes_agree(emul_lib, emul_ctx, emul_policy, C, n):
    P.routes_agree_case(emul_lib, emul_ctx, emul_policy, C, n)


def test_lines_against_the_oracle(emul_lib, emul_ctx, device_route):
    P.lines_case(emul_lib, emul_ctx, BLS12_381, 4)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_refusals(emul_lib, emul_ctx, device_route, C):
    P.refusals_case(emul_lib, emul_ctx, C, Ark355Error, EINVAL)


def test_refusals_on_the_host_route(emul_lib, emul_ctx, emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 0)
    P.refusals_case(emul_lib, emul_ctx, BLS12_381, Ark355Error, EINVAL)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_verify_batch_on_the_device_route(emul_lib, emul_ctx, device_route, C):
    pc.verify_batch_case(emul_lib, emul_ctx, C, oracle_pairing=False, light=True)


def test_default_route(emul_lib):
    """A fresh context (the session's may carry another test's policy): -1, and the crossover DESIGN.md states."""
    env = {k: os.environ.pop(k) for k in ("ARK355_PAIRING_DEVICE", "ARK355_PAIRING_DEVICE_MIN") if k in os.environ}
    try:
        ctx = emul_lib.ctx_create(0)
    finally:
        os.environ.update(env)
    try:
        assert emul_lib.ctx_get_policy(ctx, "PAIRING_DEVICE") == -1
        doc = open(os.path.join(ROOT, "DESIGN.md")).read()
        m = re.search(r"`PAIRING_DEVICE_MIN` = (\d+)", doc)
        assert m, "DESIGN.md must state the crossover as `PAIRING_DEVICE_MIN` = <value>"
        assert emul_lib.ctx_get_policy(ctx, "PAIRING_DEVICE_MIN") == int(m.group(1))
    finally:
        emul_lib.ctx_destroy(ctx)


def test_miller_loop_kernels_make_no_scratch_access():
    """On the built library (hipcc, gfx950): the Miller-loop kernels of both curves are found by name, their multiplications
    are inlined -- the branch-free runs hold at least the multiply-adds of one F_q2 product, 3 Montgomery products of 2 N^2
    32-bit multiply-adds each (N = 12 limbs on BLS12-381, 8 on BN254) -- and neither the hot loops nor anything else in them
    touches scratch memory; the accumulation keeps f in LDS."""
    import sys
    from snark_amd import build
    lib = build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import code_object_stats as cos
        st = cos.library_stats(lib)
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    for curve, limbs in (("bls12_381", 12), ("bn254", 8)):
        for k in ("pairing_lines", "pairing_accumulate", "pairing_product"):
            s = st.get("%s.%s" % (curve, k))
            assert s is not None, (curve, k, sorted(st))
            h = s["hot_block"]
            assert h["multiply_adds"] >= 3 * 2 * limbs * limbs, (curve, k, h)
            assert h["scratch_loads"] + h["scratch_stores"] == 0, (curve, k, h)
            assert s["scratch_loads"] + s["scratch_stores"] == 0, (curve, k, s)
        assert st[curve + ".pairing_accumulate"]["hot_block"]["lds"] > 0
