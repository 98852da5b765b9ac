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


@pytest.mark.parametrize("log_n", [1, 3, 7, 10, 11])
def test_ntt_fr_dev(emul_lib, emul_ctx, log_n):
    """tiny kernel and one pass (the result ends on the scratch side and is copied back), two passes (it ends in d_data)"""
    nc.ntt_dev_case(emul_lib, emul_ctx, BLS12_381, log_n, nc.HostBuffers())
