"""CPU tier: the call sequences of tests/dirty_cases.py on the emulator build, in ONE fresh context of this module.

The emulator's allocator hands out poisoned memory between guard bands (tests/emul/hip_emul.h), the library's own POISON_ALLOC is
set on top of it, and every test below leaves its residue in the context's grow-only scratch for the next one: the tests of this
module are meant to run in the order written.  GPU twin at the full sizes: tests/test_gpu_dirty.py."""
import pytest

import dirty_cases as dc
import ntt_cases as nc
import sr1cs_cases as sc
from oracle.fields import BLS12_381, BN254

CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2])


@pytest.fixture(scope="module")
def tier(emul_lib):
    ctx = dc.fresh_context(emul_lib)
    try:
        yield dc.Tier(emul_lib, ctx, sc.HostIO, nc.HostBuffers(), emul=True)
    finally:
        emul_lib.ctx_destroy(ctx)
        dc.unpoison(emul_lib)


@CURVES
def test_proofs_alternating_keys(tier, C):
    dc.proofs_sequence(tier, C)


@CURVES
def test_check_satisfied_refusals_between_proofs(tier, C):
    dc.check_satisfied_sequence(tier, C)


@GROUPS
@CURVES
def test_resident_msm(tier, C, group):
    dc.resident_msm_sequence(tier, C, group)


@GROUPS
@CURVES
def test_oneshot_msm(tier, C, group):
    dc.oneshot_msm_sequence(tier, C, group)


@CURVES
def test_ntt(tier, C):
    dc.ntt_sequence(tier, C)


@CURVES
def test_witness_map_mat_vec_is_satisfied(tier, C):
    dc.witness_map_sequence(tier, C)


@CURVES
def test_quotient_by_falling_and_rising_extension(tier, C):
    dc.quotient_sequence(tier, C)


@CURVES
def test_which_is_unsatisfied(tier, C):
    dc.which_is_unsatisfied_sequence(tier, C)


@CURVES
def test_sr1cs(tier, C):
    dc.sr1cs_sequence(tier, C)


@CURVES
def test_finalize(tier, C):
    dc.finalize_sequence(tier, C)


@CURVES
def test_setup(tier, C):
    dc.setup_sequence(tier, C)


@CURVES
def test_multi_pairing(tier, C):
    dc.pairing_sequence(tier, C)


def test_verify_each(tier):
    dc.verify_each_sequence(tier, BN254)


def test_verify_each_bytes(tier):
    dc.verify_each_bytes_sequence(tier, BN254)


@CURVES
def test_msm_after_everything_else(tier, C):
    """the families above have grown and dirtied every scratch buffer of the context: the MSM sequences once more"""
    dc.resident_msm_sequence(tier, C, 1)
    dc.oneshot_msm_sequence(tier, C, 2)
