"""Proofs as wire bytes on the CPU emulator build (see tests/verify_bytes_cases.py): the endomorphism subgroup tests, the proof
decode kernel and the drivers of `ark355_points_check`, `ark355_proofs_from_bytes` and `ark355_verify_each_bytes` compiled with
g++ against the HIP emulator, at sizes a single host thread handles."""
import pytest

import verify_bytes_cases as V
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL

CURVES = [BLS12_381, BN254]
FORMS = [True, False]


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_points_check_methods_agree_with_the_oracle(emul_lib, emul_ctx, C, group, n):
    V.points_check_case(emul_lib, emul_ctx, C, group, n)


@pytest.mark.parametrize("mode", V.MODES, ids=["none", "curve", "full"])
@pytest.mark.parametrize("comp", FORMS, ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_proofs_from_bytes(emul_lib, emul_ctx, C, comp, mode):
    V.decoder_case(emul_lib, emul_ctx, C, comp, mode, 43)


@pytest.mark.parametrize("comp", FORMS, ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_each_bytes(emul_lib, emul_ctx, emul_policy, C, comp):
    V.verify_each_bytes_case(emul_lib, emul_ctx, emul_policy, C, comp, V.FULL, 4, tamper=dict(other_c=(0,), b_off=(1,)))


def test_verify_each_bytes_one_proof_unvalidated(emul_lib, emul_ctx, emul_policy):
    V.verify_each_bytes_case(emul_lib, emul_ctx, emul_policy, BN254, False, V.NONE, 1, tamper=dict(b_off=(0,)), wire_damage=False)


def test_verify_each_bytes_without_public_inputs(emul_lib, emul_ctx, emul_policy):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    V.no_public_inputs_case(emul_lib, emul_ctx, BN254)


def test_malleated_proofs_verify_without_the_subgroup_test_and_fail_with_it(emul_lib, emul_ctx, emul_policy):
    V.malleability_case(emul_lib, emul_ctx, emul_policy, BLS12_381, True)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusals(emul_lib, emul_ctx, emul_policy, C):
    emul_policy.setenv("ARK355_PAIRING_DEVICE", 1)
    V.refusals_case(emul_lib, emul_ctx, C, EINVAL)


def test_groth16_verify_each_bytes(emul_lib):
    V.groth16_case(emul_lib, BN254)
