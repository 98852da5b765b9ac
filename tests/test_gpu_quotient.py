"""GPU tier of the quotient entries (include/ark355.h "Quotient polynomial of any predicate"): the cases of
tests/test_emul_quotient.py on the MI355X, plus the sizes only the device runs in seconds: D N = 2^11 .. 2^13 (one NTT tile and
several), the witness-map equivalence at 2^14 and 2^18 rows, and the SR1CS chain at 5000 and 2^16 source rows."""
import numpy as np
import pytest

import quotient_cases as qc
import sr1cs_cases as sc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254
from snark_amd import SR1CS

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
SHAPES = list(qc.shapes(BLS12_381))
LARGE = list(qc.large_shapes(BLS12_381))
SR1CS_INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


class DevIO:
    @staticmethod
    def to_dev(b):
        import torch
        t = torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        return t.data_ptr(), t

    @staticmethod
    def alloc(nbytes):
        import torch
        t = torch.full((max(1, nbytes),), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t.data_ptr(), t

    @staticmethod
    def read(keep, nbytes):
        return keep.cpu().numpy().tobytes()[:nbytes]


@CURVES
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_against_the_definition(gpu_lib, gpu_ctx, C, name):
    qc.shape_case(gpu_lib, gpu_ctx, C, name)


@CURVES
@pytest.mark.parametrize("name", LARGE)
def test_one_tile_and_several_against_the_definition(gpu_lib, gpu_ctx, C, name):
    qc.shape_case(gpu_lib, gpu_ctx, C, name, qc.large_shapes(C))


@CURVES
@pytest.mark.parametrize("ext", [0, 1], ids=["D1", "D2"])
@pytest.mark.parametrize("which", list(qc.POLICIES))
def test_policy_knobs_change_no_byte(gpu_lib, gpu_ctx, gpu_policy, C, which, ext):
    qc.policy_case(gpu_lib, gpu_ctx, C, gpu_policy, which, ext)


@CURVES
@pytest.mark.parametrize("name", ["circuit2", "hand-made", "random-deg3-N8"])
def test_satisfied_systems_by_exact_division_then_one_witness_changed(gpu_lib, gpu_ctx, C, name):
    qc.satisfied_case(gpu_lib, gpu_ctx, C, name)


@CURVES
def test_r1cs_shape_equals_the_witness_map(gpu_lib, gpu_ctx, C):
    qc.witness_map_case(gpu_lib, gpu_ctx, C, 1 << 14)


def test_r1cs_shape_equals_the_witness_map_at_two_to_the_eighteen(gpu_lib, gpu_ctx):
    from test_gpu_sr1cs import bench_lc_shape
    C = BLS12_381
    ell, w, mats, z = bench_lc_shape(C.r, 1 << 18)
    qc.witness_map_csr_case(gpu_lib, gpu_ctx, C, ell, w, mats, z)


@CURVES
@pytest.mark.parametrize("which", range(len(SR1CS_INSTANCES)), ids=SR1CS_INSTANCES)
def test_sr1cs_chain_on_device_pointers(gpu_lib, gpu_ctx, C, which):
    qc.sr1cs_chain_case(gpu_lib, gpu_ctx, C, DevIO, *sc.reference_instances(C)[which])


@CURVES
def test_sr1cs_chain_on_a_random_system(gpu_lib, gpu_ctx, C):
    qc.sr1cs_chain_case(gpu_lib, gpu_ctx, C, DevIO, *sc.random_instance(C, 5000, 0x5121C5 + C.curve_id))


def test_sr1cs_chain_at_two_to_the_sixteen(gpu_lib, gpu_ctx):
    """2^16 satisfied R1CS rows of the bench-LC shape: 2^17 + 1 SR1CS rows, N = 2^18"""
    from test_gpu_sr1cs import bench_lc_shape
    C, lib, ctx = BLS12_381, gpu_lib, gpu_ctx
    ell, w, mats, z = bench_lc_shape(C.r, 1 << 16)
    r1 = lib.r1cs_load(ctx, C.curve_id, 1 << 16, ell, w, mats)
    s = SR1CS.from_r1cs(lib, ctx, r1, C.curve_id, ell + w)
    try:
        zb = S._mont_bytes(C.r, z)
        assert lib.is_satisfied(ctx, r1, zb, ell + w) == -1
        qc.sr1cs_chain_on(lib, ctx, C, DevIO, s, zb, ell + w, 0x216, True)
    finally:
        s.free()
        lib.dll.ark355_r1cs_free(r1)


@CURVES
def test_explicit_log_n(gpu_lib, gpu_ctx, C):
    qc.explicit_log_n_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_handle_from_lcs(gpu_lib, gpu_ctx, C):
    qc.from_lcs_case(gpu_lib, gpu_ctx, C)


@CURVES
def test_dims_and_refusals(gpu_lib, gpu_ctx, C):
    qc.dims_and_refusals_case(gpu_lib, gpu_ctx, C)
