"""ark355_setup -- the Groth16 generator on the device -- on the MI355X: the cases of the CPU tier (tests/setup_cases.py)
plus the sizes the Python oracle cannot reach, against the oracle's C generator."""
import pytest

import setup_cases as sc
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BLS12_381, BN254]


def _ids(c):
    return c.name if hasattr(c, "name") else str(c)


@pytest.mark.parametrize("name", sc.WHOLE_KEY)
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_whole_key_equals_the_oracle_generator(gpu_lib, gpu_ctx, C, name):
    sc.whole_key_case(gpu_lib, gpu_ctx, C, name)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_resident_key_proves_and_verifies(gpu_lib, gpu_ctx, C):
    sc.resident_key_proves_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("position", [0, 1, 2], ids=["k_below_n", "k_in_input_rows", "k_beyond_n_plus_ell"])
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_tau_inside_the_domain(gpu_lib, gpu_ctx, C, position):
    tau = sc.tau_in_domain_positions(C, "mulchain13")[position]
    sc.whole_key_case(gpu_lib, gpu_ctx, C, "mulchain13", tau=tau, h_must_be_zero=True)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_heavy_and_empty_columns(gpu_lib, gpu_ctx, C):
    sc.heavy_columns_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_heavy_column_in_65536_rows(gpu_lib, gpu_ctx, C):
    sc.heavy_columns_large_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("name", ["N2", "N4"])
@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_domain_shorter_than_one_run(gpu_lib, gpu_ctx, C, name):
    sc.run_length_case(gpu_lib, gpu_ctx, C, name)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_partial_last_run(gpu_lib, gpu_ctx, C):
    sc.partial_last_run_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_argument_errors(gpu_lib, gpu_ctx, C):
    sc.argument_errors_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=_ids)
def test_moderate_size_whole_key_and_closed_form_proof(gpu_lib, gpu_ctx, C):
    sc.moderate_size_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_python_mirror_routes_agree_and_device_route_uploads_nothing(gpu_lib, curve):
    sc.python_mirror_case(gpu_lib, curve)
