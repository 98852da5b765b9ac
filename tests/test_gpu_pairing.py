"""Device pairing on the MI355X (see tests/pairing_cases.py): `ark355_multi_pairing` against oracle/pairing.py through pairs
with known discrete logarithms, the host route against the device route, and `ark355_verify_batch` on the device route up
to a batch of 4096 proofs."""
import pytest

import pairing_cases as P
import parity_cases as pc
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error

pytestmark = pytest.mark.gpu

CURVES = [BLS12_381, BN254]
_LARGE = {}


@pytest.fixture
def device_route(gpu_policy):
    gpu_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return gpu_policy


def _large_points(lib, ctx, C, n):
    """the 2^14 pairs of a curve, generated once per session"""
    key = (C.name, n)
    if key not in _LARGE:
        a, b = P.mixed_scalars(C, n, seed=41)
        _LARGE[key] = (a, b) + P.points_with_dlogs(lib, ctx, C, a, b)
    return _LARGE[key]


@pytest.fixture(scope="session")
def oracle_batches():
    """8 oracle-made proofs of one key per curve, made once per session"""
    return {C.name: P.oracle_batch(C, 8) for C in CURVES}


@pytest.mark.parametrize("n", [1, 2, 3, 67, 1000, 1 << 14])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_gt_against_the_oracle(gpu_lib, gpu_ctx, device_route, C, n):
    P.gt_case(gpu_lib, gpu_ctx, C, n, points=_large_points(gpu_lib, gpu_ctx, C, n) if n >= 1 << 14 else None)


@pytest.mark.parametrize("n", [1, 5, 300])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_routes_agree(gpu_lib, gpu_ctx, gpu_policy, C, n):
    P.routes_agree_case(gpu_lib, gpu_ctx, gpu_policy, C, n)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_lines_against_the_oracle(gpu_lib, gpu_ctx, device_route, C):
    P.lines_case(gpu_lib, gpu_ctx, C, 64)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_on_the_device_route(gpu_lib, gpu_ctx, device_route, C):
    pc.verify_batch_case(gpu_lib, gpu_ctx, C, count=6)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_4096(gpu_lib, gpu_ctx, device_route, oracle_batches, C):
    P.large_batch_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name])


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_4096_default_route_is_the_device(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    """Default policy (-1): 4099 pairs are far above PAIRING_DEVICE_MIN; the verdicts do not depend on the route."""
    gpu_policy.setenv("ARK355_PAIRING_DEVICE", -1)
    assert gpu_lib.ctx_get_policy(gpu_ctx, "PAIRING_DEVICE_MIN") < 4096
    P.large_batch_case(gpu_lib, gpu_ctx, C, oracle_batches[C.name], total=4096, tamper=4000)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(gpu_lib, gpu_ctx, device_route, C):
    P.refusals_case(gpu_lib, gpu_ctx, C, Ark355Error, EINVAL)


def test_default_route(gpu_lib, gpu_ctx):
    import os
    import re
    from conftest import ROOT
    if "ARK355_PAIRING_DEVICE" not in os.environ:
        assert gpu_lib.ctx_get_policy(gpu_ctx, "PAIRING_DEVICE") == -1
    if "ARK355_PAIRING_DEVICE_MIN" not in os.environ:
        m = re.search(r"`PAIRING_DEVICE_MIN` = (\d+)", open(os.path.join(ROOT, "DESIGN.md")).read())
        assert m and gpu_lib.ctx_get_policy(gpu_ctx, "PAIRING_DEVICE_MIN") == int(m.group(1))
