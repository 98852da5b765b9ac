"""Wire formats behind the C ABI on the CPU emulator build (see tests/wire_cases.py)."""
import pytest

import wire_cases as W
from oracle.fields import BLS12_381, BN254


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_point_codecs(emul_lib, emul_ctx, C):
    W.points_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("C,compressed", [(BLS12_381, False), (BLS12_381, True), (BN254, True)],
                         ids=["bls-uncompressed", "bls-compressed", "bn-compressed"])
def test_key_stream_to_proof_bytes(emul_lib, emul_ctx, C, compressed):
    W.key_stream_case(emul_lib, emul_ctx, C, n=12, compressed=compressed)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_validation_modes(emul_lib, emul_ctx, C):
    W.validation_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("compressed", [False, True])
def test_c_oracle_key_stream_loads_and_proves(emul_lib, emul_ctx, compressed):
    """The stream builder of the BASELINE-size GPU test (tests/test_gpu_wire_large.py: raw key of the oracle's C generator ->
    cbase.pk_stream) at a size the emulator handles: ark355_pk_load_bytes -> ark355_prove == cbase.prove on the raw key."""
    import o3_cases as O
    from oracle import serialize as Z, synthetic as S
    from oracle.c import cbase
    C = BLS12_381
    inst = S.mulchain_csr(C.r, 20)
    n, ell, w, mats, z = inst
    pk = O.oracle_key(C, inst)
    stream = cbase.pk_stream(C, pk, compressed)
    pkh = emul_lib.pk_load_bytes(emul_ctx, C.curve_id, stream, compressed=compressed, validate=1)
    rh = emul_lib.r1cs_load(emul_ctx, C.curve_id, n, ell, w, mats)
    try:
        zb = S._mont_bytes(C.r, z)
        got = emul_lib.prove(emul_ctx, pkh, rh, zb, len(z), Z.fr_canon(C, 5), Z.fr_canon(C, 6), emul_lib.sizes(C.curve_id))
        assert got == O.oracle_prove(C, inst, zb, pk, 5, 6)
    finally:
        emul_lib.dll.ark355_pk_free(pkh)
        emul_lib.dll.ark355_r1cs_free(rh)


# ---- against the oracle's decoder (oracle/serialize.py g1_decode / g2_decode): exact bytes, exact status ---------------------------
FORMS = [(1, True), (1, False), (2, True), (2, False)]
FORM_IDS = ["g1-compressed", "g1-uncompressed", "g2-compressed", "g2-uncompressed"]


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_constructed_edge_points(emul_lib, emul_ctx, C):
    W.edge_points_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_differential_fuzz(emul_lib, emul_ctx, C):
    """(half of the GPU tier's count per source: the conditions on the oracle's verdicts hold at either size)"""
    W.fuzz_case(emul_lib, emul_ctx, C, scale=0.5)


@pytest.mark.parametrize("group,comp", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_batch_counts(emul_lib, emul_ctx, C, group, comp):
    """The counts around one and two wavefronts in every format, without the subgroup test (a 255-bit multiplication per point,
    which the smaller cases above run); 1000 and 2^16 + 1 points in the one format that costs the emulator neither that nor a
    square root.  The GPU tier runs all counts in all formats with the subgroup test."""
    whole = C is BN254 and group == 1 and not comp
    W.batch_counts_case(emul_lib, emul_ctx, C, group, comp, counts=W.BATCH_COUNTS if whole else W.BATCH_COUNTS[:-2],
                        modes=(W.VALIDATE_CURVE,))


@pytest.mark.parametrize("C,group,comp", [(BLS12_381, 1, True), (BN254, 1, False)], ids=["bls-g1-compressed", "bn-g1-uncompressed"])
def test_smallest_failing_index_is_reported(emul_lib, emul_ctx, C, group, comp):
    """One format with a subgroup test and the one group without (the two plans of the case); the GPU tier runs all eight,
    where lanes really finish out of order."""
    W.first_failure_case(emul_lib, emul_ctx, C, group, comp)


@pytest.mark.parametrize("C,compressed", [(BLS12_381, False), (BLS12_381, True), (BN254, False), (BN254, True)],
                         ids=["bls-uncompressed", "bls-compressed", "bn-uncompressed", "bn-compressed"])
def test_key_stream_names_the_damaged_point(emul_lib, emul_ctx, C, compressed):
    W.key_stream_damage_case(emul_lib, emul_ctx, C, n=12, compressed=compressed)
