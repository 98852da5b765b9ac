"""CPU tier of the Square R1CS entry points (include/ark355.h "Square R1CS"): the library's own kernels and host code over the
single-threaded HIP emulator, against the transliterated adapter of tests/sr1cs_cases.py -- the cases of
tests/test_gpu_sr1cs.py at sizes the emulator runs in seconds."""
import pytest

import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


@CURVES
@pytest.mark.parametrize("which", range(len(INSTANCES)), ids=INSTANCES)
def test_against_the_transliterated_adapter(emul_lib, emul_ctx, C, which):
    sc.against_transliteration_case(emul_lib, emul_ctx, C, sc.HostIO, which)


@CURVES
@pytest.mark.parametrize("rows", [70, 300])                 # 70 rows: a partial second wave of a 64-lane wave
def test_random_systems(emul_lib, emul_ctx, C, rows):
    sc.random_case(emul_lib, emul_ctx, C, sc.HostIO, rows, seed=0x5121C5 + rows)


@CURVES
def test_edges(emul_lib, emul_ctx, C):
    sc.edges_case(emul_lib, emul_ctx, C, sc.HostIO, n_same=70)


@CURVES
def test_satisfaction_transfers(emul_lib, emul_ctx, C):
    sc.satisfaction_case(emul_lib, emul_ctx, C, 70)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    sc.refusal_case(emul_lib, emul_ctx, C)
