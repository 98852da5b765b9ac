"""GPU tier of ark355_gr1cs_from_lcs (include/ark355.h "finalize() on the device"): the cases of tests/test_emul_lcmap.py on the
MI355X -- the bench.rs circuit at 2^14 rows and a random system of 5000 LCs where the emulator runs 300 -- plus one 2^18-row
instance of the bench.rs shape from a numpy generator that emits the flat LC map directly, checked against entries that exist
without this one (ark355_r1cs_load, ark355_r1cs_mat_vec, ark355_is_satisfied)."""
import numpy as np
import pytest

import lcmap_cases as lc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254
from snark_amd import _binding as B

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
CIRCUITS = ["circuit2", "circuit1", "example"]


@CURVES
@pytest.mark.parametrize("which", range(len(CIRCUITS)), ids=CIRCUITS)
def test_reference_circuits(gpu_lib, gpu_ctx, C, which):
    lc.reference_circuit_case(gpu_lib, gpu_ctx, C, which)


@CURVES
def test_bench_rs_circuit(gpu_lib, gpu_ctx, C):
    lc.bench_rs_case(gpu_lib, gpu_ctx, C, 1 << 14)


@CURVES
def test_handmade_system_through_both_compaction_paths(gpu_lib, gpu_ctx, gpu_policy, C):
    lc.handmade_case(gpu_lib, gpu_ctx, C, gpu_policy)


@CURVES
def test_random_systems(gpu_lib, gpu_ctx, C):
    lc.random_case(gpu_lib, gpu_ctx, C, 5000, seed=0x1C3A9)


@CURVES
def test_random_system_through_the_long_path(gpu_lib, gpu_ctx, gpu_policy, C):
    gpu_policy.setenv("ARK355_LCS_ROW_LDS_MAX", 8)
    lc.random_case(gpu_lib, gpu_ctx, C, 5000, seed=0x1C3A9)


@CURVES
@pytest.mark.parametrize("mode", [1, 2], ids=["outline_r1cs", "outline_sr1cs"])
def test_outlining(gpu_lib, gpu_ctx, C, mode):
    lc.outline_case(gpu_lib, gpu_ctx, C, mode, n_random=1000)


@CURVES
def test_edges(gpu_lib, gpu_ctx, C):
    lc.edges_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    lc.refusal_case(gpu_lib, gpu_ctx, C)


def bench_rs_shape(n, seed=0x355):
    """The shape of examples/bench.rs:22-83 as flat arrays, vectorised: every variable is a witness (three up front, three per
    row), row i draws from the ten most recent ones; A_i and B_i are LCs of 1..10 coefficient-one terms, an even row also has an
    extra LC of A_i's size that A_i references, C_i is a bare variable.  Returns the LC map (offsets, packed variables,
    coefficient indices -- all 0, i.e. one), the three argument columns, and the same system as CSR for ark355_r1cs_load
    (repeated columns are summed there)."""
    rng = np.random.default_rng(seed)
    rows = np.arange(n)
    have = 3 + 3 * rows                                    # variables before row i
    cur = np.minimum(have, 10)
    lower = have - cur
    size_a, size_b = rng.integers(1, 11, n), rng.integers(1, 11, n)
    even = rows % 2 == 0
    # LCs in map order: [extra_i (even i)], A_i, B_i; LC 0 is the empty one
    kind = np.tile(np.array([0, 1, 2]), n)                 # 0 extra, 1 A, 2 B
    row_of = np.repeat(rows, 3)
    keep = (kind != 0) | even[row_of]
    kind, row_of = kind[keep], row_of[keep]
    sizes = np.where(kind == 2, size_b[row_of], size_a[row_of]) + ((kind == 1) & even[row_of])
    offsets = np.concatenate([[0, 0], np.cumsum(sizes)]).astype(np.uint64)
    lc_index = 1 + np.arange(len(kind))
    e_lc = np.repeat(np.arange(len(kind)), sizes)          # the LC (position in `kind`) of every entry
    e_row = row_of[e_lc]
    wit = lower[e_row] + rng.integers(0, 1 << 30, len(e_lc)) % cur[e_row]
    vars_ = (np.uint64(B.VAR_WITNESS << B.VAR_TAG_SHIFT) | wit.astype(np.uint64))
    last = np.cumsum(sizes) - 1                            # the last entry of an even row's A is the reference to its extra
    ref_a = (kind == 1) & even[row_of]
    vars_[last[ref_a]] = np.uint64(B.VAR_LC << B.VAR_TAG_SHIFT) | (lc_index[ref_a] - 1).astype(np.uint64)
    is_ref = np.zeros(len(e_lc), dtype=bool)
    is_ref[last[ref_a]] = True
    c_wit = lower + rng.integers(0, 1 << 30, n) % cur
    lc_tag = np.uint64(B.VAR_LC << B.VAR_TAG_SHIFT)
    args = [lc_tag | lc_index[kind == 1].astype(np.uint64), lc_tag | lc_index[kind == 2].astype(np.uint64),
            np.uint64(B.VAR_WITNESS << B.VAR_TAG_SHIFT) | c_wit.astype(np.uint64)]
    ell, w = 1, 3 + 3 * n

    def csr(mask):
        counts = np.bincount(e_row[mask], minlength=n)
        return (np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), (ell + wit[mask]).astype(np.uint32))
    in_a = (kind[e_lc] != 2) & ~is_ref                     # extra_i and A_i are adjacent in the map: the mask keeps rows together
    mats = [csr(in_a), csr(kind[e_lc] == 2), (np.arange(n + 1, dtype=np.uint64), (ell + c_wit).astype(np.uint32))]
    return ell, w, offsets, vars_, np.zeros(len(vars_), dtype=np.uint32), args, mats


def test_two_to_the_eighteen_rows_against_the_existing_entries(gpu_lib, gpu_ctx):
    against_existing_entries(gpu_lib, gpu_ctx, 1 << 18)


def against_existing_entries(lib, ctx, n):
    """the handle ark355_gr1cs_r1cs gives for the finalized system and ark355_r1cs_load of the same generator's CSR agree on
    A z, B z, C z (byte for byte) and on ark355_is_satisfied: all variables one, all witnesses zero (satisfied), random values"""
    C = BLS12_381
    p = C.r
    ell, w, offsets, vars_, coeffs, args, mats = bench_rs_shape(n)
    m = ell + w
    one = S._mont_bytes(p, [1])
    pool = one + S._mont_bytes(p, [p - 1])
    r1cs_poly = (S._mont_bytes(p, [1, p - 1]), np.array([0, 2, 3], np.uint32), np.array([0, 1, 2], np.uint32), np.array([1, 1, 1], np.uint32))
    g = lib.gr1cs_from_lcs(ctx, C.curve_id, ell, w, offsets, vars_, coeffs, pool, [("R1CS", 3, n) + r1cs_poly + (args,)])
    r_dev = r_ref = None
    try:
        assert lib.gr1cs_dims(g) == (ell, w, 1)
        arity, rows, nnz = lib.gr1cs_pred_dims(g, 0)
        assert (arity, rows) == (3, n) and nnz[2] == n and all(0 < nnz[k] <= len(mats[k][1]) for k in range(2))   # merged repeats
        r_dev = lib.gr1cs_r1cs(ctx, g)
        r_ref = lib.r1cs_load(ctx, C.curve_id, n, ell, w, [(rp, col, one * len(col)) for rp, col in mats])
        rnd = np.random.default_rng(0x18)
        body = rnd.integers(0, 256, (w, 32), dtype=np.uint8)
        body[:, 31] = 0                                                                # below the modulus
        zs = [one * m, one + bytes(32 * w), one + body.tobytes()]
        for zb in zs:
            first = lib.is_satisfied(ctx, r_ref, zb, m)
            assert lib.is_satisfied(ctx, r_dev, zb, m) == first
            assert lib.mat_vec(ctx, r_dev, zb, m, n, 32) == lib.mat_vec(ctx, r_ref, zb, m, n, 32)
        assert lib.is_satisfied(ctx, r_ref, zs[1], m) == -1
    finally:
        for r in (r_dev, r_ref):
            if r is not None:
                lib.dll.ark355_r1cs_free(r)
        lib.gr1cs_free(g)
