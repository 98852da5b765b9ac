"""Proofs as wire bytes on the MI355X (see tests/verify_bytes_cases.py): the endomorphism subgroup tests against `[r]P` and the
oracle across the ends of a wave and a second workgroup, `ark355_proofs_from_bytes` byte for byte against the oracle's decoder
with every kind of defect in every position, `ark355_verify_each_bytes` on both routes, past the chunk, without public inputs,
the malleated proofs, the refusals and the Python layer."""
import pytest

import verify_bytes_cases as V
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL

pytestmark = pytest.mark.gpu

CURVES = [BLS12_381, BN254]
FORMS = [True, False]
COUNTS = [1, 43, 130]          # 3 * 43 = 129 lanes cross one workgroup of the decode kernel


@pytest.fixture
def device_route(gpu_policy):
    gpu_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    return gpu_policy


@pytest.mark.parametrize("n", [1, 64, 65, 129])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_points_check_methods_agree_with_the_oracle(gpu_lib, gpu_ctx, C, group, n):
    V.points_check_case(gpu_lib, gpu_ctx, C, group, n)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("mode", V.MODES, ids=["none", "curve", "full"])
@pytest.mark.parametrize("comp", FORMS, ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_proofs_from_bytes(gpu_lib, gpu_ctx, C, comp, mode, count):
    V.decoder_case(gpu_lib, gpu_ctx, C, comp, mode, count)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("comp", FORMS, ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_bytes(gpu_lib, gpu_ctx, gpu_policy, C, comp, count):
    V.verify_each_bytes_case(gpu_lib, gpu_ctx, gpu_policy, C, comp, V.FULL, count)


@pytest.mark.parametrize("mode", [V.NONE, V.CURVE], ids=["none", "curve"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_bytes_weaker_modes(gpu_lib, gpu_ctx, gpu_policy, C, mode):
    V.verify_each_bytes_case(gpu_lib, gpu_ctx, gpu_policy, C, False, mode, 43)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_bytes_past_the_chunk(gpu_lib, gpu_ctx, device_route, C):
    V.past_the_chunk_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_bytes_without_public_inputs(gpu_lib, gpu_ctx, device_route, C):
    V.no_public_inputs_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("comp", FORMS, ids=["compressed", "uncompressed"])
def test_malleated_proofs_verify_without_the_subgroup_test_and_fail_with_it(gpu_lib, gpu_ctx, gpu_policy, comp):
    V.malleability_case(gpu_lib, gpu_ctx, gpu_policy, BLS12_381, comp)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(gpu_lib, gpu_ctx, device_route, C):
    V.refusals_case(gpu_lib, gpu_ctx, C, EINVAL)


def test_groth16_verify_each_bytes(gpu_lib):
    V.groth16_case(gpu_lib, BLS12_381)
