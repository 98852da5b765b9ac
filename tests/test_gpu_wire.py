"""Wire formats behind the C ABI on the GPU (see tests/wire_cases.py): device point codecs and the end-to-end path
ProvingKey bytes -> ark355_pk_load_bytes -> ark355_prove -> proof bytes == the oracle's."""
import pytest

import wire_cases as W
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_point_codecs(gpu_lib, gpu_ctx, C):
    W.points_case(gpu_lib, gpu_ctx, C, n=40)


@pytest.mark.parametrize("C,compressed", [(BLS12_381, False), (BLS12_381, True), (BN254, False), (BN254, True)],
                         ids=["bls-uncompressed", "bls-compressed", "bn-uncompressed", "bn-compressed"])
def test_key_stream_to_proof_bytes(gpu_lib, gpu_ctx, C, compressed):
    W.key_stream_case(gpu_lib, gpu_ctx, C, n=150, compressed=compressed)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_validation_modes(gpu_lib, gpu_ctx, C):
    """Validate::Yes semantics on the device decoders and on the proof path: subgroup membership, canonical infinity,
    flag combinations (tests/wire_cases.py)."""
    W.validation_case(gpu_lib, gpu_ctx, C)


# ---- against the oracle's decoder (oracle/serialize.py g1_decode / g2_decode): exact bytes, exact status ---------------------------
FORMS = [(1, True), (1, False), (2, True), (2, False)]
FORM_IDS = ["g1-compressed", "g1-uncompressed", "g2-compressed", "g2-uncompressed"]


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_constructed_edge_points(gpu_lib, gpu_ctx, C):
    """Twist points with a real x^3 + b' (both branches of the Fq2 root, both tie-breaks of the Fq2 ordering), x = 0,
    coordinates q - 1 / q / q + 1 / all ones in every slot, BN254's ignored sign bit: device codecs and the proof codecs of the
    host against the oracle."""
    W.edge_points_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_differential_fuzz(gpu_lib, gpu_ctx, C):
    W.fuzz_case(gpu_lib, gpu_ctx, C)


@pytest.mark.parametrize("group,comp", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_batch_counts(gpu_lib, gpu_ctx, C, group, comp):
    """1, 63 .. 65, 127 .. 129, 1000 and 2^16 + 1 points both ways against the C oracle's encoder"""
    W.batch_counts_case(gpu_lib, gpu_ctx, C, group, comp)


@pytest.mark.parametrize("group,comp", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_smallest_failing_index_is_reported(gpu_lib, gpu_ctx, C, group, comp):
    W.first_failure_case(gpu_lib, gpu_ctx, C, group, comp)


@pytest.mark.parametrize("C,compressed", [(BLS12_381, False), (BLS12_381, True), (BN254, False), (BN254, True)],
                         ids=["bls-uncompressed", "bls-compressed", "bn-uncompressed", "bn-compressed"])
def test_key_stream_names_the_damaged_point(gpu_lib, gpu_ctx, C, compressed):
    W.key_stream_damage_case(gpu_lib, gpu_ctx, C, n=12, compressed=compressed)
