"""CPU tier: the cold 32-bit XYZZ group law (curve.cuh, wave_reduce_sum / batch_to_affine_kernel of msm_impl.cuh) on the emulator
build, driven through equal, opposite and empty operands by the designed inputs of tests/grouplaw_cases.py: ark355_xyzz_sum over
hand-built XYZZ operands, ark355_fixed_base_mul on both routes with scalars that collide with the window table, structured group
transforms and column gathers, and verification batches whose prepared inputs double, cancel, start and end at infinity.  The
integer-side assertions of every design (branch classes per butterfly level, infinity sets, collider hits) run first, with the
library never called; the expected points come from the oracle alone.  GPU twin: tests/test_gpu_grouplaw.py."""
import numpy as np
import pytest

import grouplaw_cases as gc
from oracle.fields import BLS12_381, BN254

CURVES = [BLS12_381, BN254]
GROUPS = [1, 2]
_ids = lambda v: getattr(v, "name", str(v))      # noqa: E731


def _to_dev(b):        # emulator: "device" pointers are host pointers
    a = np.frombuffer(b, dtype=np.uint8).copy()
    return a.ctypes.data, a


@pytest.fixture(scope="module")
def tier(emul_lib, emul_ctx):
    return gc.Tier(emul_lib, emul_ctx, _to_dev)


# ---- on integers alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_sum_model_covers_every_class_at_every_level(C):
    """Six classes in the serial phase and at each of the six butterfly levels; a level with three or more classes in one wave."""
    divergent = gc.assert_sum_coverage(C.r)
    assert any(d.startswith("fuzz") for d, _ in divergent)
    for design in gc.SUM_DESIGNS:
        for count in gc.SUM_COUNTS:
            gc.assert_sum_design(design, count, gc.sum_multipliers(design, count), C.r)
    assert gc.SUM_COUNTS[-1] > 192


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_fixed_base_designs_on_integers(C):
    """The colliders meet acc == +-T[31][d]; BN254's first colliding top digit is 49."""
    for n in gc.FB_NS:
        inf = gc.assert_fb_design(C, n, gc.fb_scalars(C, n))
        assert {0, 15, 16, 127, n - 1} | set(range(64, 80)) <= set(inf)
        assert max(gc.fb_scalars(C, n, below_r=True)) < C.r
    if C is BN254:
        assert gc.fb_collider(C.r) == (2 * 49 * (1 << 248) - C.r, 49)


@pytest.mark.parametrize("log_n", [1, 2, 3, 4])
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_transform_designs_on_integers(C, log_n):
    for design in gc.HB_DESIGNS:
        gc.assert_hb_design(C, log_n, design, gc.hb_inputs(C, log_n, design))


@pytest.mark.parametrize("key", list(gc.VERIFY_KEYS))
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_verify_batches_on_integers(C, key):
    vk, proofs, inputs, want = gc.verify_batch(C, key)
    assert len(proofs) == len(inputs) == len(want) and True in want and False in want


# ---- 1. ark355_xyzz_sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", gc.SUM_DESIGNS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_xyzz_sum_designs(tier, C, group, design):
    gc.sum_case(tier, C, group, design)


# ---- 2. ark355_fixed_base_mul ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.FB_BASES)
@pytest.mark.parametrize("n", gc.FB_NS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_fixed_base_both_routes(tier, C, group, n, name):
    gc.fixed_base_case(tier, C, group, n, name)


@pytest.mark.parametrize("entry", ["dev", "dev-mont"])
@pytest.mark.parametrize("n", gc.FB_NS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_fixed_base_dev_both_routes(tier, C, group, n, entry):
    gc.fixed_base_case(tier, C, group, n, "P", entry=entry)


# ---- 3. ark355_hbasis_transform --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", gc.HB_DESIGNS)
@pytest.mark.parametrize("log_n", [1, 2, 3, 4])
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_transform_designs(tier, C, log_n, design):
    gc.transform_case(tier, C, log_n, design)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_transform_constant_64(tier, C):
    gc.transform_case(tier, C, 6, "constant")


# ---- 4. ark355_hbasis_gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", gc.GATHER_DESIGNS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_gather_hand_built(tier, C, design):
    gc.gather_hand_built_case(tier, C, design)


@pytest.mark.parametrize("design", gc.GATHER_DESIGNS)
@pytest.mark.parametrize("length", gc.HEAVY_LENGTHS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_gather_heavy_column(tier, C, length, design):
    gc.gather_heavy_case(tier, C, length + 1, design)


# ---- 5. ark355_verify_each / ark355_verify_each_pvk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 0])
@pytest.mark.parametrize("key", list(gc.VERIFY_KEYS))
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_verify_each_prepared_inputs(tier, emul_policy, C, key, route):
    gc.verify_case(tier, emul_policy, C, key, route)
