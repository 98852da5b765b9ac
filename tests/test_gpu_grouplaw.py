"""GPU tier (-m gpu): the cold 32-bit XYZZ group law (curve.cuh, wave_reduce_sum / batch_to_affine_kernel of msm_impl.cuh) on the
device, driven through equal, opposite and empty operands by the designed inputs of tests/grouplaw_cases.py.  Every other device
test feeds this code sums of random points, for which P + P, P + (-P), O + P, P + O and O + O are never taken and two equal points
in different representations never meet.  The emulator tier (tests/test_emul_grouplaw.py) runs lanes one after another as host
code; what only this tier sees is the gfx950 code: the out-of-line xyzz_add of each field called under divergence -- some lanes of a
wave doubling, some cancelling, some passing an empty operand --, its operands travelling through xyzz_shfl_xor and by-reference
stack slots, xyzz_madd_ni's out-of-line doubling in the window walk and in the unit-coefficient gather.

Sizes are the smallest at which each path exists: the second and third trip of xyzz_sum_kernel's lane loop (65, 129, 200 partials),
the table route of the fixed-base multiplication (512 scalars), a partial workgroup and a partial batch of 16 (530), a heavy column
of less than one chunk and of three."""
import numpy as np
import pytest

import grouplaw_cases as gc
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BLS12_381, BN254]
GROUPS = [1, 2]
_ids = lambda v: getattr(v, "name", str(v))      # noqa: E731


def _to_dev(b):
    import torch
    t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.fixture(scope="module")
def tier(gpu_lib, gpu_ctx):
    return gc.Tier(gpu_lib, gpu_ctx, _to_dev)


# ---- 1. ark355_xyzz_sum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", gc.SUM_DESIGNS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_xyzz_sum_designs(tier, C, group, design):
    """Every count and both choices of lambda; the model's coverage of classes per level is asserted once per curve."""
    if design == gc.SUM_DESIGNS[0] and group == 1:
        gc.assert_sum_coverage(C.r)
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
def test_verify_each_prepared_inputs(tier, gpu_policy, C, key, route):
    gc.verify_case(tier, gpu_policy, C, key, route)
