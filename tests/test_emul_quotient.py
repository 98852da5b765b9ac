"""CPU tier of the quotient entries (include/ark355.h "Quotient polynomial of any predicate"): the library's own kernels and
host code over the single-threaded HIP emulator, against the references of tests/quotient_cases.py -- the cases of
tests/test_gpu_quotient.py at sizes the emulator runs in seconds."""
import pytest

import quotient_cases as qc
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
SHAPES = list(qc.shapes(BLS12_381))
SR1CS_INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


@CURVES
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_against_the_definition(emul_lib, emul_ctx, C, name):
    qc.shape_case(emul_lib, emul_ctx, C, name)


@CURVES
@pytest.mark.parametrize("ext", [0, 1], ids=["D1", "D2"])
@pytest.mark.parametrize("which", list(qc.POLICIES))
def test_policy_knobs_change_no_byte(emul_lib, emul_ctx, emul_policy, C, which, ext):
    qc.policy_case(emul_lib, emul_ctx, C, emul_policy, which, ext)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-N8"])
def test_satisfied_systems_by_exact_division_then_one_witness_changed(emul_lib, emul_ctx, C, name):
    qc.satisfied_case(emul_lib, emul_ctx, C, name)


@CURVES
@pytest.mark.parametrize("n", [13, 1030])
def test_r1cs_shape_equals_the_witness_map(emul_lib, emul_ctx, C, n):
    qc.witness_map_case(emul_lib, emul_ctx, C, n)


@CURVES
@pytest.mark.parametrize("which", range(len(SR1CS_INSTANCES)), ids=SR1CS_INSTANCES)
def test_sr1cs_chain_on_device_pointers(emul_lib, emul_ctx, C, which):
    qc.sr1cs_chain_case(emul_lib, emul_ctx, C, sc.HostIO, *sc.reference_instances(C)[which])


@CURVES
@pytest.mark.parametrize("rows", [70, 300])
def test_sr1cs_chain_on_random_systems(emul_lib, emul_ctx, C, rows):
    qc.sr1cs_chain_case(emul_lib, emul_ctx, C, sc.HostIO, *sc.random_instance(C, rows, 0x5121C5 + rows + C.curve_id))


@CURVES
def test_explicit_log_n(emul_lib, emul_ctx, C):
    qc.explicit_log_n_case(emul_lib, emul_ctx, C)


@CURVES
def test_handle_from_lcs(emul_lib, emul_ctx, C):
    qc.from_lcs_case(emul_lib, emul_ctx, C)


@CURVES
def test_dims_and_refusals(emul_lib, emul_ctx, C):
    qc.dims_and_refusals_case(emul_lib, emul_ctx, C)
