"""CPU tier of the GR1CS entry points (include/ark355.h "GR1CS"): the library's own kernels and host code over the
single-threaded HIP emulator, against the oracle -- the same cases as tests/test_gpu_gr1cs.py at sizes the emulator runs in
seconds (every instance <= 2^10 rows)."""
import pytest

import gr1cs_cases as gc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
def test_reference_circuit1(emul_lib, emul_ctx, C):
    gc.circuit1_case(emul_lib, emul_ctx, C)


@CURVES
def test_label_order_beats_registration_order_and_row_index(emul_lib, emul_ctx, C):
    gc.label_order_case(emul_lib, emul_ctx, C)


@CURVES
def test_random_systems(emul_lib, emul_ctx, C):
    gc.random_systems_case(emul_lib, emul_ctx, C, rows=70)        # 70 rows: a partial second wave of a 64-lane workgroup


def test_random_systems_many_rows(emul_lib, emul_ctx):
    gc.random_systems_case(emul_lib, emul_ctx, BLS12_381, rows=300, seed=77)


def test_polynomial_at_the_limits(emul_lib, emul_ctx):
    gc.limit_polynomial_case(emul_lib, emul_ctx, BN254)


@CURVES
def test_r1cs_through_the_general_path(emul_lib, emul_ctx, C):
    gc.r1cs_general_case(emul_lib, emul_ctx, C, *S.mulchain_direct(C.r, 13), prove=True)
    gc.r1cs_general_case(emul_lib, emul_ctx, C, *S.cs_to_instance(S.dummy_cs(C.r, 16)))          # empty rows
    gc.r1cs_general_case(emul_lib, emul_ctx, C, *S.cs_to_instance(S.bench_lc_cs(C.r, 20)))       # general coefficients
    gc.r1cs_refusal_case(emul_lib, emul_ctx, C)


@CURVES
def test_reference_sr1cs_predicate(emul_lib, emul_ctx, C):
    gc.sr1cs_case(emul_lib, emul_ctx, C, rows=300)


@CURVES
def test_refusals(emul_lib, emul_ctx, C):
    gc.refusal_case(emul_lib, emul_ctx, C)


def test_three_predicate_system_walked_in_full(emul_lib, emul_ctx):
    gc.scale_case(emul_lib, emul_ctx, BLS12_381, 1 << 10, sample=64, full_walk=True)
