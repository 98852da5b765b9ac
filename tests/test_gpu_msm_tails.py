"""GPU tier (-m gpu): the MSM tail kernels (tails28_impl.cuh) on the device, driven through doublings, cancellations and empties by
the designed inputs of tests/msm_tail_cases.py.  Every other device test feeds the tails sums of random points: two bucket sums are
then never equal or opposite and no row or column is at infinity, so the cold paths of add28 / add28_g2 (the doubling inside a wave
butterfly, the pair-wide votes under the divergence of the merge, the empty flag through add_xor and the shortened butterfly,
store_canonical of an empty bit sum) and the LDS hand-over of the heavy merge ran without a test that would notice a wrong answer.

Window sizes: the smallest at which each shape of msm_selsum28_kernel exists -- G1 (64 items per wave) at 11 (32 x 32: shortened
butterfly, no lane chain), 14 (128 x 64: rows chained twice, columns one item per lane) and 16 (256 x 128: chains of four and two);
G2 (32 items per wave) at 11 (one item per lane pair), 13 (chains of two) and 14 (unequal split).  CPU twin at the small sizes:
tests/test_emul_msm_tails.py."""
import numpy as np
import pytest

import msm_tail_cases as tc
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
GROUPS = [1, 2]
SHAPES = [(1, 11), (1, 14), (1, 16), (2, 11), (2, 13), (2, 14)]          # (group, window size)
_ids = lambda v: getattr(v, "name", str(v))      # noqa: E731


def _to_dev(b):
    import torch
    t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.fixture(scope="module")
def tier(gpu_lib, gpu_ctx):
    return tc.Tier(gpu_lib, gpu_ctx, _to_dev, min_span=48)


@pytest.mark.parametrize("design", tc.MATRIX_DESIGNS)
@pytest.mark.parametrize("group,c", SHAPES)
def test_matrix_designs(tier, gpu_policy, group, c, design):
    tc.matrix_case(tier, gpu_policy, BLS12_381, group, c, design)


@pytest.mark.parametrize("design", ["constant", "fuzz-1", "fuzz-2", "fuzz-3"])
@pytest.mark.parametrize("group,c", [(1, 11), (1, 16), (2, 11), (2, 14)])
def test_matrix_designs_bn254(tier, gpu_policy, group, c, design):
    tc.matrix_case(tier, gpu_policy, BN254, group, c, design)


@pytest.mark.parametrize("pack", [0, 1])
@pytest.mark.parametrize("group,c", [(1, 14), (2, 13)])
def test_matrix_designs_row_formats(tier, gpu_policy, group, c, pack):
    """PACK_ROWS 0 and 1: both accumulation kernels hand the tails their slots."""
    tc.matrix_case(tier, gpu_policy, BLS12_381, group, c, "fuzz-2", pack=pack)
    tc.matrix_case(tier, gpu_policy, BLS12_381, group, c, "alternating", pack=pack)


def test_matrix_design_montgomery_scalars(tier, gpu_policy):
    tc.matrix_case(tier, gpu_policy, BLS12_381, 1, 14, "fuzz-3", mont=1)


@pytest.mark.parametrize("group", GROUPS)
def test_strided_tables(tier, gpu_policy, group):
    """MSM_C = 13 with TABLE_STRIDE = 2: `constant` in bucket set 0, `alternating` in set 1, combined by the host's Horner."""
    tc.strided_case(tier, gpu_policy, BLS12_381, group, 13)


@pytest.mark.parametrize("dmax", [7, 8])
@pytest.mark.parametrize("design", tc.ONESHOT_DESIGNS)
@pytest.mark.parametrize("group", GROUPS)
def test_oneshot_designs(tier, group, design, dmax):
    tc.oneshot_case(tier, BLS12_381, group, design, dmax)


# ---- merge designs: MSM_SEG = 16, c = 11; a bucket is heavy over more than 48 segment boundaries ----------------------------------
MERGE_ON = [(BLS12_381, 1), (BLS12_381, 2), (BN254, 1)]
PLAIN_RUNS = (3, 40)
HEAVY_RUNS = (64, 512)          # 64: one G1 wave full, three empty in LDS; 512: two equal runs per G1 lane, four equal wave sums


@pytest.mark.parametrize("front", [0, 5])
@pytest.mark.parametrize("runs", PLAIN_RUNS)
@pytest.mark.parametrize("C,group", MERGE_ON, ids=_ids)
def test_merge_equal_runs(tier, gpu_policy, C, group, runs, front):
    tc.merge_case(tier, gpu_policy, C, group, tc.SEG * runs, front=front)


@pytest.mark.parametrize("front", [0, 5])
@pytest.mark.parametrize("runs", HEAVY_RUNS)
@pytest.mark.parametrize("C,group", MERGE_ON, ids=_ids)
def test_merge_heavy_equal_runs(tier, gpu_policy, C, group, runs, front):
    tc.merge_case(tier, gpu_policy, C, group, tc.SEG * runs, front=front, heavy=True)


@pytest.mark.parametrize("signs", ["a", "b", "balanced"])
@pytest.mark.parametrize("runs", PLAIN_RUNS + HEAVY_RUNS)
@pytest.mark.parametrize("C,group", MERGE_ON, ids=_ids)
def test_merge_sign_fuzz(tier, gpu_policy, C, group, runs, signs):
    """Each entry P or -P: the runs are small multiples of P, in any order, some of them empty; `balanced`: the bucket ends at
    infinity, and the MSM with it."""
    tc.merge_case(tier, gpu_policy, C, group, tc.SEG * runs, front=0, signs=signs, heavy=runs in HEAVY_RUNS)
    tc.merge_case(tier, gpu_policy, C, group, tc.SEG * runs, front=5, signs=signs, heavy=runs in HEAVY_RUNS)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=_ids)
@pytest.mark.parametrize("group", GROUPS)
def test_xyzz_sum_equal_opposite_empty(tier, group, C):
    tc.xyzz_case(tier, C, group)
