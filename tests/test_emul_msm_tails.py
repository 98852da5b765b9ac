"""CPU tier: the MSM tail kernels (tails28_impl.cuh) on the emulator build, driven through doublings, cancellations and empties by
the designed inputs of tests/msm_tail_cases.py -- bucket-to-bucket and run-to-run additions whose operands are equal, opposite or
infinity, which sums of random points never are.  Every design asserts its property on the integer bucket matrix before the library
is called; the answer comes from a known discrete log.

The emulator twin runs the resident window size 11 (32 x 32 buckets: one item per G1 lane, shortened butterfly; 32 items = one per
G2 lane pair) and the one-shot window 4 for every design, and G2 at 13 (lane chains of two) for `constant`.  This build takes a
bucket as heavy from five segments on at these shapes (ARK_MSM_HEAVY_SPAN = 2, twice the average span of 2), so the plain merge
designs use 3 and 4 runs and 40 runs already reach msm_merge_heavy28_kernel.  GPU twin, with the larger window sizes:
tests/test_gpu_msm_tails.py."""
import numpy as np
import pytest

import msm_tail_cases as tc
from oracle.fields import BLS12_381, BN254

GROUPS = [1, 2]


def _to_dev(b):        # emulator: "device" pointers are host pointers
    a = np.frombuffer(b, dtype=np.uint8).copy()
    return a.ctypes.data, a


@pytest.fixture(scope="module")
def tier(emul_lib, emul_ctx):
    return tc.Tier(emul_lib, emul_ctx, _to_dev, min_span=2)


@pytest.mark.parametrize("c", [4, 11, 13, 14, 16])
def test_reference_sums(c):
    """The reference checks itself: for every design the bit sums recompose to sum (b + 1) M_b, and the named property holds on the
    multipliers themselves."""
    for design in tc.MATRIX_DESIGNS:
        m = tc.multipliers(design, 1 << (c - 1))
        tc.tail_sums(m, c)
        if c > 4 or not design.startswith("single"):
            tc.assert_design(design, m, c)
    assert tc.split(11) == (5, 5) and tc.split(14) == (7, 6) and tc.split(16) == (8, 7) and tc.split(4) == (2, 1)


@pytest.mark.parametrize("design", tc.MATRIX_DESIGNS)
@pytest.mark.parametrize("group", GROUPS)
def test_matrix_designs(tier, emul_policy, group, design):
    tc.matrix_case(tier, emul_policy, BLS12_381, group, 11, design)


def test_matrix_constant_g2_lane_chain(tier, emul_policy):
    """G2 at c = 13: 64 items per row and column, so the second item of every lane pair's chain doubles too."""
    tc.matrix_case(tier, emul_policy, BLS12_381, 2, 13, "constant")


@pytest.mark.parametrize("design", ["constant", "fuzz-1", "fuzz-2", "fuzz-3"])
@pytest.mark.parametrize("group", GROUPS)
def test_matrix_designs_bn254(tier, emul_policy, group, design):
    tc.matrix_case(tier, emul_policy, BN254, group, 11, design)


@pytest.mark.parametrize("pack", [0, 1])
@pytest.mark.parametrize("group", GROUPS)
def test_matrix_designs_row_formats(tier, emul_policy, group, pack):
    """PACK_ROWS 0 and 1: both accumulation kernels hand the tails their slots."""
    tc.matrix_case(tier, emul_policy, BLS12_381, group, 11, "fuzz-2", pack=pack)


def test_matrix_design_montgomery_scalars(tier, emul_policy):
    tc.matrix_case(tier, emul_policy, BLS12_381, 1, 11, "fuzz-3", mont=1)


@pytest.mark.parametrize("group", GROUPS)
def test_strided_tables(tier, emul_policy, group):
    """Two bucket sets at c = 11: `constant` in set 0, `alternating` in set 1, combined by the host's Horner."""
    tc.strided_case(tier, emul_policy, BLS12_381, group, 11)


@pytest.mark.parametrize("dmax", [7, 8])
@pytest.mark.parametrize("design", tc.ONESHOT_DESIGNS)
@pytest.mark.parametrize("group", GROUPS)
def test_oneshot_designs(tier, group, design, dmax):
    tc.oneshot_case(tier, BLS12_381, group, design, dmax)


# (curve, group) of the merge designs
MERGE_ON = [(BLS12_381, 1), (BLS12_381, 2), (BN254, 1)]
_ids = lambda v: getattr(v, "name", str(v))      # noqa: E731


@pytest.mark.parametrize("front", [0, 5])
@pytest.mark.parametrize("runs", [3, 4])
@pytest.mark.parametrize("C,group", MERGE_ON, ids=_ids)
def test_merge_equal_runs(tier, emul_policy, C, group, runs, front):
    tc.merge_case(tier, emul_policy, C, group, tc.SEG * runs, front=front)


# 256 runs need a table of 4096 rows: once per group
HEAVY = [(C, g, runs, front) for C, g in MERGE_ON for runs in (40, 64) for front in (0, 5)] + [(BLS12_381, 1, 256, 0), (BLS12_381, 2, 256, 0)]


@pytest.mark.parametrize("C,group,runs,front", HEAVY, ids=_ids)
def test_merge_heavy_equal_runs(tier, emul_policy, C, group, runs, front):
    """40 runs: part of one wave; 64: one wave full and three empty in the LDS sum (G1); 256: one run per G1 lane, every butterfly
    step doubles and the four wave sums that meet in LDS are equal (two equal runs per G2 lane pair)."""
    tc.merge_case(tier, emul_policy, C, group, tc.SEG * runs, front=front, heavy=True)


# every shape above with one seed, the balanced bucket (it ends at infinity, and the MSM with it) on one plain and two heavy shapes
SIGN_FUZZ = ([(3, 0, "a", False), (3, 5, "b", False), (4, 0, "b", False), (4, 5, "a", False), (3, 0, "balanced", False)]
             + [(40, 0, "a", True), (40, 5, "b", True), (64, 0, "b", True), (64, 5, "a", True), (40, 0, "balanced", True),
                (64, 0, "balanced", True)])


@pytest.mark.parametrize("runs,front,signs,heavy", SIGN_FUZZ)
@pytest.mark.parametrize("C,group", MERGE_ON, ids=_ids)
def test_merge_sign_fuzz(tier, emul_policy, C, group, runs, front, signs, heavy):
    """Each entry P or -P: the runs are small multiples of P, in any order, some of them empty."""
    tc.merge_case(tier, emul_policy, C, group, tc.SEG * runs, front=front, signs=signs, heavy=heavy)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=_ids)
@pytest.mark.parametrize("group", GROUPS)
def test_xyzz_sum_equal_opposite_empty(tier, group, C):
    tc.xyzz_case(tier, C, group)
