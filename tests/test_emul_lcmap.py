"""CPU tier of ark355_gr1cs_from_lcs (include/ark355.h "finalize() on the device"): the library's own kernels and host code over
the single-threaded HIP emulator, against oracle/r1cs.py's finalize() + to_matrices() and the transliterated outliner of
tests/lcmap_cases.py -- the cases of tests/test_gpu_lcmap.py at sizes the emulator runs in seconds."""
import pytest

import lcmap_cases as lc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
CIRCUITS = ["circuit2", "circuit1", "example"]


@CURVES
@pytest.mark.parametrize("which", range(len(CIRCUITS)), ids=CIRCUITS)
def test_reference_circuits(emul_lib, emul_ctx, C, which):
    lc.reference_circuit_case(emul_lib, emul_ctx, C, which)


@CURVES
def test_bench_rs_circuit(emul_lib, emul_ctx, C):
    lc.bench_rs_case(emul_lib, emul_ctx, C, 300)


@CURVES
def test_handmade_system_through_both_compaction_paths(emul_lib, emul_ctx, emul_policy, C):
    lc.handmade_case(emul_lib, emul_ctx, C, emul_policy)


@CURVES
@pytest.mark.parametrize("n_lcs", [70, 300])                # 70 LCs: a partial second wave of a 64-lane wave
def test_random_systems(emul_lib, emul_ctx, C, n_lcs):
    lc.random_case(emul_lib, emul_ctx, C, n_lcs, seed=0x1C3A9 + n_lcs)


@CURVES
def test_random_system_through_the_long_path(emul_lib, emul_ctx, emul_policy, C):
    emul_policy.setenv("ARK355_LCS_ROW_LDS_MAX", 8)
    lc.random_case(emul_lib, emul_ctx, C, 300, seed=0x1C3A9 + 300)


@CURVES
@pytest.mark.parametrize("mode", [1, 2], ids=["outline_r1cs", "outline_sr1cs"])
def test_outlining(emul_lib, emul_ctx, C, mode):
    lc.outline_case(emul_lib, emul_ctx, C, mode, n_random=70)


@CURVES
def test_edges(emul_lib, emul_ctx, C):
    lc.edges_case(emul_lib, emul_ctx, C)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    lc.refusal_case(emul_lib, emul_ctx, C)
