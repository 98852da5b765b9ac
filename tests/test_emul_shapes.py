"""A small subset of the shape and operand cases of tests/test_gpu_shapes.py over the CPU emulator build: it keeps the case
code (closed forms, guard handling, the diagonal system) exercised on a machine without a GPU.  It does NOT stand in for the
GPU run: the emulator has no concurrency inside a workgroup and compiles the portable multiplier."""
import pytest

import field_edge_cases as fe
import ntt_cases as nc
from oracle.fields import BLS12_381, BN254


@pytest.mark.parametrize("log_n", [4, 6, 12])
def test_ntt_structured_inputs(emul_lib, emul_ctx, log_n):
    nc.structured_case(emul_lib, emul_ctx, BLS12_381, log_n)


@pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
def test_multiplier_patterns_fr(emul_lib, emul_ctx, C):
    fe.diagonal_pairs_case(emul_lib, emul_ctx, C)


@pytest.mark.parametrize("C,group", [(BLS12_381, 1), (BLS12_381, 2), (BN254, 1), (BN254, 2)],
                         ids=["bls12_381-g1", "bls12_381-g2", "bn254-g1", "bn254-g2"])
def test_multiplier_patterns_fq_points(emul_lib, emul_ctx, emul_policy, C, group):
    """Points whose coordinates have pattern Montgomery images through the wire codecs, fixed_base_mul, the on-curve check of
    multi_pairing and the MSM paths (tests/field_edge_cases.py): here the portable multiplier, on the GPU the assembly one."""
    import numpy as np

    def to_dev(b):      # emulator: "device" pointers are host pointers
        a = np.frombuffer(b, dtype=np.uint8).copy()
        return a.ctypes.data, a
    fe.pattern_points_group_case(emul_lib, emul_ctx, emul_policy, C, group, to_dev)


@pytest.mark.parametrize("log_n", [1, 3, 7, 10, 11])
def test_ntt_fr_dev(emul_lib, emul_ctx, log_n):
    """tiny kernel and one pass (the result ends on the scratch side and is copied back), two passes (it ends in d_data)"""
    nc.ntt_dev_case(emul_lib, emul_ctx, BLS12_381, log_n, nc.HostBuffers())
