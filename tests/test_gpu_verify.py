"""What the two routes of the pairing entries share (see tests/verify_cases.py), on the MI355X: `ark355_verify_batch` host
route against device route at 1, 61 and 62 proofs -- with the key's three pairs exactly one 64-lane workgroup of the
Miller-loop kernels, and one workgroup plus one lane -- and the refusal texts."""
import pytest

import pairing_cases as P
import verify_cases as V
from oracle.fields import BLS12_381, BN254
from snark_amd._binding import EINVAL, Ark355Error

pytestmark = pytest.mark.gpu

CURVES = [BLS12_381, BN254]


@pytest.fixture(scope="module")
def oracle_batches():
    """8 oracle-made proofs of one key per curve, made once"""
    return {C.name: P.oracle_batch(C, 8) for C in CURVES}


@pytest.mark.parametrize("count", [1, 61, 62])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_verify_batch_routes_agree(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C, count):
    V.verify_batch_routes_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name], count)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_refusal_texts(gpu_lib, gpu_ctx, gpu_policy, oracle_batches, C):
    V.refusal_texts_case(gpu_lib, gpu_ctx, gpu_policy, C, oracle_batches[C.name], Ark355Error, EINVAL)
