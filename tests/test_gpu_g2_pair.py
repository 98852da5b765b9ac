"""GPU tier (-m gpu): the lane-pair G2 bucket accumulation (msm_accumulate_g2l28_kernel / msm_accumulate_g2l28p_kernel) against
the independent C oracle, byte for byte.

Resident-table G2 MSMs (ark355_bases_load + ark355_msm_dev) at 2^10 and 2^12 terms on both curves, under every workgroup size
of the accumulation kernel (policy ACC_THREADS 64 / 128 / 256: one, two and four waves share the kernel's LDS) and both row
formats (policy PACK_ROWS 0 / 1: the plain walk with zz, zzz, x, y in LDS on BLS12-381, and the parked-flush walk with the
accumulator in registers), with scalar vectors that drive the mixed addition through its cases:
  uniform      general additions
  equal        one heavy bucket per window; on the duplicated bases P + P (the doubling path)
  cancel       pairs k, r - k; on the duplicated bases the two digits are negatives of each other: P - P, then a re-opened bucket
  infinity     a base vector with points at infinity (single ones and a run), uniform scalars
and one 2^12-constraint proof per curve against the oracle's prover.  References are computed once per (curve, size)."""
import random

import numpy as np
import pytest

import o3_cases as O
from oracle import serialize as Z, synthetic as S
from oracle.c import cbase
from oracle.fields import BLS12_381, BN254

pytestmark = pytest.mark.gpu
CURVES = [BLS12_381, BN254]
DISTS = ("uniform", "equal", "cancel", "infinity")

_REF = {}


def _reference(C, n):
    """{dist: (bases, scalars, expected)} for one curve and size; the oracle's MSM runs once per entry and session."""
    key = (C.name, n)
    if key in _REF:
        return _REF[key]
    psz = 4 * C.fq_bytes
    plain = O.bases(C, 2, n)                                       # P_i = (i + 1) G
    dup = bytearray(plain)
    for i in range(0, n // 2, 2):                                  # first half: P_{i+1} = P_i
        dup[(i + 1) * psz:(i + 2) * psz] = dup[i * psz:(i + 1) * psz]
    dup = bytes(dup)
    holes = bytearray(dup)
    for i in list(range(3, n, 5)) + list(range(n // 2, n // 2 + 40)):
        holes[i * psz:(i + 1) * psz] = bytes(psz)
    holes = bytes(holes)
    rnd = random.Random(0x62 + n)
    ks = [rnd.randrange(1, C.r) for _ in range(n // 2)]
    cancel = b"".join(Z.fr_canon(C, k) + Z.fr_canon(C, C.r - k) for k in ks)
    cases = {
        "uniform": (dup, O.scalars(C, n, "uniform", seed=n + 1)),
        "equal": (dup, O.scalars(C, n, "equal", seed=n + 2)),
        "cancel": (dup, cancel),
        "infinity": (holes, O.scalars(C, n, "uniform", seed=n + 3)),
    }
    _REF[key] = {d: (b, s, cbase.msm(C, 2, b, s, n)) for d, (b, s) in cases.items()}
    # the duplicated pairs of `cancel` sum to nothing, the distinct ones do not: the expected point is a real one
    assert any(_REF[key]["cancel"][2])
    return _REF[key]


def _to_dev(b):
    import torch
    t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.mark.parametrize("acc_threads", [64, 128, 256])
@pytest.mark.parametrize("pack", [0, 1], ids=["unpacked", "packed"])
@pytest.mark.parametrize("log_n", [10, 12])
@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_resident_g2_msm_vs_oracle(gpu_lib, gpu_ctx, gpu_policy, C, log_n, pack, acc_threads):
    n = 1 << log_n
    ref = _reference(C, n)
    psz = gpu_lib.sizes(C.curve_id)["g2"]
    gpu_policy.setenv("ARK355_PACK_ROWS", pack)                    # read when the tables are made
    gpu_policy.setenv("ARK355_ACC_THREADS", acc_threads)           # read by every call
    handles = {}
    try:
        for dist in DISTS:
            bases, scalars, expect = ref[dist]
            if bases not in handles:
                handles[bases] = gpu_lib.bases_load(gpu_ctx, C.curve_id, 2, bases, n)
            ptr, keep = _to_dev(scalars)
            got = gpu_lib.msm_dev(gpu_ctx, handles[bases], ptr, n, 0, psz)
            assert got == expect, (C.name, n, dist, "PACK_ROWS", pack, "ACC_THREADS", acc_threads)
    finally:
        for h in handles.values():
            gpu_lib.dll.ark355_bases_free(h)


@pytest.mark.parametrize("C", CURVES, ids=lambda c: c.name)
def test_prove_2p12_vs_oracle(gpu_lib, gpu_ctx, C):
    """A 2^12-constraint proof (its B query runs through the lane-pair kernel) byte-equal to the oracle's prover, and through
    the Groth16 equation."""
    O.check_instance(gpu_lib, gpu_ctx, C, S.mulchain_csr(C.r, 1 << 12), [(0x51ED, C.r - 7)])
