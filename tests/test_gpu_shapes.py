"""GPU tier (-m gpu): the SHAPES of the transform kernels and the operands of the hand-written multiplier on real hardware.

The emulator (tests/emul) runs one thread at a time and hands control over at barriers, and it compiles the portable
multiplier: a missing __syncthreads(), an LDS tile two waves overwrite, or a wrong carry in the inline-assembly chain of
csrc/field.cuh shows only here.  Rows of the planner's table and the parametrised ids that run them (radices; p_log):

  log_n 1, 2      tiny kernel                       test_ntt_every_plan[*-1], [*-2]; test_ntt_fr_dev[*-1], [*-2]
  log_n 3 .. 9    one pass [log_n]                  test_ntt_every_plan[*-3] .. [*-9]; structured: 4, 5, 6, 9
  log_n 10 .. 18  two passes [5,5] [6,5] [6,6] [7,6] [7,7] [8,7] [8,8] [9,8] [9,9]
                                                    test_ntt_every_plan[*-10] .. [*-18]; structured: 12, 14, 16
  log_n 19, 20    three passes [5,9,5] [6,8,6]      test_ntt_every_plan[*-19], [*-20]
  log_n 24        [9,6,9], no direct twiddle table  test_ntt_2p24[*]; test_ntt_fr_dev[bls12_381-24]
  log_n 25        [8,9,8], likewise                 test_ntt_2p25
  fused seams (witness map), radix 5 .. 9           test_witness_map_every_domain[*-5] .. [*-10], [*-12], [*-14], [*-16], [*-18], [*-19]
  policies                                          test_ntt_policy_sweep[*], test_witness_map_nofuse_equals_fused

Every comparison is against the C oracle (oracle/c) or Python integers, on whole vectors."""
import contextlib

import numpy as np
import pytest

import field_edge_cases as fe
import ntt_cases as nc
import o3_cases as O
import parity_cases as pc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BLS12_381, BN254]
_name = lambda v: getattr(v, "name", str(v))          # noqa: E731


def to_dev(b):
    import torch
    t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


class TorchBuffers:
    """ntt_cases.HostBuffers over torch device tensors, for the context's own stream (None) and a torch.cuda.Stream.  The
    stream contract of include/ark355.h: `*_dev` entries read their buffers on the library's streams, so whatever produced them
    is complete before the call -- except that ark355_ntt_fr_dev, handed the PRODUCER's stream, orders itself on it."""

    def __init__(self):
        import torch
        self.torch = torch
        self.streams = (None, torch.cuda.Stream())

    def _on(self, stream):
        return self.torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()

    def guarded(self, payload, nbytes, fill, stream):
        torch = self.torch
        with self._on(stream):
            t = torch.full((nbytes + 2 * nc.GUARD,), fill, dtype=torch.uint8, device="cuda")
            if payload is not None:
                t[nc.GUARD:nc.GUARD + nbytes].copy_(torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()), non_blocking=True)
        return t.data_ptr() + nc.GUARD, t

    def before_call(self, stream):
        if stream is None:
            self.torch.cuda.synchronize()

    def stream_handle(self, stream):
        return stream.cuda_stream if stream is not None else None

    def after_call(self, stream):
        if stream is None:
            self.torch.cuda.synchronize()          # the context's stream belongs to the library: wait for the device
        else:
            stream.synchronize()

    def read(self, buf, stream):
        return buf.cpu().numpy()


@pytest.fixture(scope="module")
def torch_buffers(gpu_lib):
    return TorchBuffers()


# ---- 1: every transform plan, whole vector, four modes ------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(1, 21))
@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_ntt_every_plan(gpu_lib, gpu_ctx, C, log_n):
    nc.ntt_full_case(gpu_lib, gpu_ctx, C, log_n)


@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_ntt_2p24(gpu_lib, gpu_ctx, C):
    """2^24 = 2^9 x 2^6 x 2^9: the first domain whose first pass has no direct twiddle table (ntt_twiddle_kernel), and the
    domain of the 2^23-constraint proofs; four modes on both curves"""
    nc.ntt_full_case(gpu_lib, gpu_ctx, C, 24)


def test_ntt_2p25(gpu_lib, gpu_ctx):
    """One size beyond: 2^25 = 2^8 x 2^9 x 2^8 (1 GiB of Fr), forward and coset inverse"""
    nc.ntt_full_case(gpu_lib, gpu_ctx, BLS12_381, 25, modes=((0, 0), (1, 1)))


# ---- 2: inputs whose answer needs no oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 5, 6, 9, 12, 14, 16])
@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_ntt_structured_inputs(gpu_lib, gpu_ctx, C, log_n):
    nc.structured_case(gpu_lib, gpu_ctx, C, log_n)


# ---- 3: the planner's policies --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [(("NTT_RMAX", 2),), (("NTT_RMAX", 3),), (("NTT_RMAX", 4),), (("NTT_RMAX", 5),),
                                    (("NTT_DIRECT_MAX", 4),), (("NTT_DIRECT_MAX", 4), ("NTT_RMAX", 3)), (("NTT_NOFUSE", 1),)],
                         ids=lambda p: ",".join("%s=%d" % kv for kv in p))
def test_ntt_policy_sweep(gpu_lib, gpu_ctx, gpu_policy, policy):
    """Up to five passes of radix 2^1 .. 2^5 (NTT_RMAX), the composed twiddles of domains without a direct table
    (NTT_DIRECT_MAX; the policy is read at every call and table look-ups respect it, so the session's context serves), the
    unfused inverse -> coset path (NTT_NOFUSE): transforms at 2^1 .. 2^12 and R1CS operations + witness maps up to 2^14."""
    for name, value in policy:
        gpu_policy.setenv("ARK355_" + name, str(value))
        assert gpu_lib.ctx_get_policy(gpu_ctx, name) == value
    nc.policy_sweep_case(gpu_lib, gpu_ctx, BLS12_381, seed=sum(v for _, v in policy))
    pc.ntt_case(gpu_lib, gpu_ctx, BN254, 7, seed=3)
    pc.ntt_case(gpu_lib, gpu_ctx, BN254, 11, seed=3)


@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_witness_map_nofuse_equals_fused(gpu_lib, gpu_ctx, gpu_policy, C):
    nc.nofuse_equals_fused_case(gpu_lib, gpu_ctx, gpu_policy, C)


# ---- 4: ark355_ntt_fr_dev -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,log_n", [(BLS12_381, k) for k in list(range(1, 21)) + [24]] + [(BN254, k) for k in (1, 2, 4, 9, 11, 16, 19, 20)],
                         ids=_name)
def test_ntt_fr_dev(gpu_lib, gpu_ctx, torch_buffers, C, log_n):
    """ark355_ntt_fr_dev in place on torch device buffers with 4 KiB guard regions, once on the context's stream and once
    on a torch.cuda.Stream: pass counts 1, 2, 3 and the tiny kernel (odd counts end on the scratch side and are copied back)."""
    nc.ntt_dev_case(gpu_lib, gpu_ctx, C, log_n, torch_buffers)


# ---- 5: the witness map at every domain size ------------------------------------------------------------------------------------
_DIST = {10: (2, 4), 14: (2, 4), 17: (2, 4), 18: (2, 4)}


@pytest.mark.parametrize("C,log_N", [(BLS12_381, k) for k in range(3, 20)] + [(BN254, k) for k in range(3, 19)], ids=_name)
def test_witness_map_every_domain(gpu_lib, gpu_ctx, C, log_N):
    """Every coefficient of h against cb_witness_map, satisfied and unsatisfied assignments, for a circuit that fills the
    domain to within a row (n + ell = N - 1) and one just above half of it (n + ell = N / 2 + 1); at four sizes also the
    distributed map over 2 and 4 simulated ranks."""
    N = 1 << log_N
    for n in sorted({N - 3, N // 2 - 1}):
        inst = S.mulchain_csr(C.r, n)
        assert N // 2 < inst[0] + inst[1] <= N
        O.check_witness_map_full(gpu_lib, gpu_ctx, C, inst, dist_worlds=_DIST.get(log_N, ()) if n == N - 3 else ())


# ---- 6: device-pointer MSM entries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_resident_bases_partial_and_sum(gpu_lib, gpu_ctx, C, group):
    """ark355_msm_dev_partial + ark355_xyzz_sum (and ark355_msm_dev over a prefix of the rows): two partials as on the
    emulator; four partials of which one is the point at infinity; count = 0 and count = 1."""
    pc.resident_partial_and_sum_case(gpu_lib, gpu_ctx, C, group, to_dev, cuts=(0, 20, 50) if group == 1 else (0, 8, 20), prefix=7, seed=9)
    pc.resident_partial_and_sum_case(gpu_lib, gpu_ctx, C, group, to_dev, cuts=(0, 9, 30, 41, 64) if group == 1 else (0, 5, 12, 20, 26),
                                     prefix=1, seed=19, zero_partial=2)
    pc.resident_count_zero_and_one_case(gpu_lib, gpu_ctx, C, group, to_dev)


@pytest.mark.parametrize("group,n", [(1, 320), (1, 1100), (2, 256)])
@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_msm_dev_montgomery_scalars(gpu_lib, gpu_ctx, C, group, n):
    """ark355_msm_dev(scalars_mont = 1) == scalars_mont = 0 == the known discrete log, scalars around (r - 1) / 2"""
    pc.resident_known_dlog_case(gpu_lib, gpu_ctx, C, group, n, to_dev)


# ---- 7: multiplier operands that sampling never produces ------------------------------------------------------------------------
@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_multiplier_patterns_fr(gpu_lib, gpu_ctx, C):
    """Fr::mul on the device (inline-assembly chain) on all ordered pairs of 17 Montgomery-image patterns:
    ark355_r1cs_mat_vec, ark355_is_satisfied, ark355_gr1cs_eval against Python integers"""
    fe.diagonal_pairs_case(gpu_lib, gpu_ctx, C)


def test_multiplier_patterns_fq_bn254_g1(gpu_lib, gpu_ctx):
    """Fq / Fp28 through points: BN254 G1 (cofactor 1: every curve point is in the subgroup) points whose x is a pattern,
    through ark355_msm_g1, bases_load + msm_dev, fixed_base_mul and both wire formats, with scalars up to r - 1.  The other
    three groups have a cofactor: their pattern points lie outside the prime-order subgroup and go through the cases below."""
    fe.pattern_points_case(gpu_lib, gpu_ctx, BN254, to_dev)


def test_multiplier_patterns_fq_bls12_381_g1(gpu_lib, gpu_ctx, gpu_policy):
    """The 12-limb multiplier of the production curve (and its radix-2^28 form, through resident tables) on points of
    BLS12-381 G1 whose x is a pattern: on the curve, outside the prime-order subgroup, so only through paths that are plain
    group law -- wire codecs, fixed_base_mul, the on-curve check of multi_pairing, MSMs with scalars up to (r - 1) / 2."""
    fe.pattern_points_group_case(gpu_lib, gpu_ctx, gpu_policy, BLS12_381, 1, to_dev)


@pytest.mark.parametrize("C", CURVES, ids=_name)
def test_multiplier_patterns_fq2_g2(gpu_lib, gpu_ctx, gpu_policy, C):
    """Fq2 on both curves: twist points whose x.c0 and x.c1 are patterns (each with itself and with its neighbour)"""
    fe.pattern_points_group_case(gpu_lib, gpu_ctx, gpu_policy, C, 2, to_dev)


def test_multiplier_patterns_fq_bn254_g1_on_curve_check(gpu_lib, gpu_ctx, gpu_policy):
    """The paths test_multiplier_patterns_fq_bn254_g1 does not take: VALIDATE_CURVE / VALIDATE_NONE, the on-curve check of
    multi_pairing, PACK_ROWS 0"""
    fe.pattern_points_group_case(gpu_lib, gpu_ctx, gpu_policy, BN254, 1, to_dev)
