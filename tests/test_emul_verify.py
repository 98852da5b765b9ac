"""What the two routes of the pairing entries share (see tests/verify_cases.py), on the CPU emulator build: phase lines,
verify_batch verdicts and refusal texts, at sizes a single host thread handles."""
import pytest

import pairing_cases as P
import verify_cases as V
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error

CURVES = [BLS12_381, BN254]


@pytest.fixture(scope="module")
def small_batches():
    """2 oracle-made proofs of one key per curve"""
    return {C.name: P.oracle_batch(C, 2) for C in CURVES}


def test_phase_lines(emul_lib, emul_ctx, emul_policy, capfd, small_batches):
    V.trace_case(emul_lib, emul_ctx, emul_policy, capfd, BN254, small_batches[BN254.name])


@pytest.mark.parametrize("count", [1, 2])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_routes_agree(emul_lib, emul_ctx, emul_policy, small_batches, C, count):
    V.verify_batch_routes_case(emul_lib, emul_ctx, emul_policy, C, small_batches[C.name], count)


def test_refusal_texts(emul_lib, emul_ctx, emul_policy, small_batches):
    V.refusal_texts_case(emul_lib, emul_ctx, emul_policy, BLS12_381, small_batches[BLS12_381.name], Ark355Error, EINVAL)
