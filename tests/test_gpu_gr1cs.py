"""GPU tier of the GR1CS entry points (include/ark355.h "GR1CS"): the cases of tests/test_emul_gr1cs.py on the MI355X at larger
sizes, plus the 2^20-constraint system over three predicates."""
import pytest

import gr1cs_cases as gc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)


@CURVES
def test_reference_circuit1(gpu_lib, gpu_ctx, C):
    gc.circuit1_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_label_order_beats_registration_order_and_row_index(gpu_lib, gpu_ctx, C):
    gc.label_order_case(gpu_lib, gpu_ctx, C, rows=300)


@CURVES
def test_random_systems(gpu_lib, gpu_ctx, C):
    gc.random_systems_case(gpu_lib, gpu_ctx, C, rows=1000)


def test_polynomial_at_the_limits(gpu_lib, gpu_ctx):
    gc.limit_polynomial_case(gpu_lib, gpu_ctx, BN254, rows=300)
    gc.limit_polynomial_case(gpu_lib, gpu_ctx, BLS12_381, rows=70)


@CURVES
def test_r1cs_through_the_general_path(gpu_lib, gpu_ctx, C):
    gc.r1cs_general_case(gpu_lib, gpu_ctx, C, *S.mulchain_direct(C.r, 29), prove=True)
    gc.r1cs_general_case(gpu_lib, gpu_ctx, C, *S.mulchain_direct(C.r, 3000))
    gc.r1cs_general_case(gpu_lib, gpu_ctx, C, *S.cs_to_instance(S.dummy_cs(C.r, 64)))            # empty rows
    gc.r1cs_general_case(gpu_lib, gpu_ctx, C, *S.cs_to_instance(S.bench_lc_cs(C.r, 200)))        # general coefficients
    gc.r1cs_refusal_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_reference_sr1cs_predicate(gpu_lib, gpu_ctx, C):
    gc.sr1cs_case(gpu_lib, gpu_ctx, C, rows=5000)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    gc.refusal_case(gpu_lib, gpu_ctx, C)


def test_three_predicate_system_walked_in_full(gpu_lib, gpu_ctx):
    gc.scale_case(gpu_lib, gpu_ctx, BN254, 1 << 14, full_walk=True)


def test_two_to_the_twenty_constraints_over_three_predicates(gpu_lib, gpu_ctx):
    gc.scale_case(gpu_lib, gpu_ctx, BLS12_381, 1 << 20)
