"""GPU tier (-m gpu): the call sequences of tests/dirty_cases.py on the MI355X, in ONE fresh context of this module created
with POISON_ALLOC set (every device and pinned buffer of the library starts as 0xA5 bytes, whatever fresh device memory holds on
the machine -- which these tests neither measure nor depend on).  Every test leaves its residue in the context's grow-only scratch
for the next one: the tests are meant to run in the order written.  Every step is compared with the oracle.  CPU twin, same
sequences at smaller sizes, where a poisoned index costs a process and not a device: tests/test_emul_dirty.py."""
import pytest

import dirty_cases as dc
from test_gpu_shapes import TorchBuffers          # device buffers of the NTT cases: one definition for both modules
from test_gpu_sr1cs import DevIO                   # device memory of the `_dev` entries, likewise
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
GROUPS = pytest.mark.parametrize("group", [1, 2])


@pytest.fixture(scope="module")
def tier(gpu_lib):
    ctx = dc.fresh_context(gpu_lib)
    try:
        yield dc.Tier(gpu_lib, ctx, DevIO, TorchBuffers(), emul=False)
    finally:
        gpu_lib.ctx_destroy(ctx)
        dc.unpoison(gpu_lib)


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
