"""GPU tier of the Square R1CS entry points (include/ark355.h "Square R1CS"): the cases of tests/test_emul_sr1cs.py on the MI355X
at 5000 rows where the emulator runs 70 or 300 (several workgroups across the scans), plus one 2^18-row instance of the bench-LC
shape checked against entries that exist without the adapter (ark355_r1cs_mat_vec, ark355_is_satisfied)."""
import random

import numpy as np
import pytest

import sr1cs_cases as sc
from oracle import synthetic as S
from oracle.fields import BLS12_381, BN254
from snark_amd import SR1CS

pytestmark = pytest.mark.gpu
CURVES = pytest.mark.parametrize("C", [BLS12_381, BN254], ids=lambda c: c.name)
INSTANCES = ["mulchain-13", "dummy-16", "bench_lc-20", "circuit2", "hand-made"]


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
@pytest.mark.parametrize("which", range(len(INSTANCES)), ids=INSTANCES)
def test_against_the_transliterated_adapter(gpu_lib, gpu_ctx, C, which):
    sc.against_transliteration_case(gpu_lib, gpu_ctx, C, DevIO, which)


@CURVES
def test_random_systems(gpu_lib, gpu_ctx, C):
    sc.random_case(gpu_lib, gpu_ctx, C, DevIO, 5000, seed=0x5121C5)


@CURVES
def test_edges(gpu_lib, gpu_ctx, C):
    sc.edges_case(gpu_lib, gpu_ctx, C, DevIO, n_same=5000)


@CURVES
def test_satisfaction_transfers(gpu_lib, gpu_ctx, C):
    sc.satisfaction_case(gpu_lib, gpu_ctx, C, 5000)


@CURVES
def test_refusals(gpu_lib, gpu_ctx, C):
    sc.refusal_case(gpu_lib, gpu_ctx, C)


def bench_lc_shape(p, n, seed=0x355):
    """The shape of S3 "bench-LC" (oracle/synthetic.py: A and B are linear combinations of 1..10 terms over the 10 most recent
    variables with general coefficients, C a fresh witness that makes the row hold), in CSR and in about three seconds at 2^18
    rows: oracle.synthetic.bench_lc_csr spends half a minute there, in its own random stream and its restated LinearCombination.
    Coefficients come from a palette of 1024 random field elements, so their Montgomery images are 1024 conversions."""
    rnd = random.Random(seed)
    palette = [rnd.randrange(1, p) for _ in range(1024)]
    images = np.frombuffer(S._mont_bytes(p, palette), dtype=np.uint8).reshape(1024, 32)
    ell = 2
    z = [1, 7] + [rnd.randrange(p) for _ in range(10)]
    recent = list(range(2, 12)) + [1]                      # ten witnesses, then the input x: the pool of bench.rs
    rps, cols, cfs = ([0], [0]), ([], []), ([], [])
    getbits = rnd.getrandbits
    for _ in range(n):
        vals = [0, 0]
        window = recent[-10:]
        for k in range(2):
            acc = 0
            for _ in range(1 + getbits(16) % 10):
                ci, j = getbits(10), window[getbits(16) % 10]
                cols[k].append(j)
                cfs[k].append(ci)
                acc += palette[ci] * z[j]
            rps[k].append(len(cols[k]))
            vals[k] = acc % p
        recent.append(len(z))
        z.append(vals[0] * vals[1] % p)
    one = np.frombuffer(S._mont_bytes(p, [1]), dtype=np.uint8)
    mats = [(np.array(rps[k], dtype=np.uint64), np.array(cols[k], dtype=np.uint32), images[np.array(cfs[k])].tobytes())
            for k in range(2)]
    mats.append((np.arange(n + 1, dtype=np.uint64), np.arange(12, 12 + n, dtype=np.uint32), np.tile(one, n).tobytes()))
    return ell, len(z) - ell, mats, z


def test_two_to_the_eighteen_rows_against_the_existing_entries(gpu_lib, gpu_ctx):
    """M0 z' = Az +- Bz, M1 z' = 4 Cz + (Az - Bz)^2 and (Az - Bz)^2 on a 4096-row sample, with Az, Bz, Cz from
    ark355_r1cs_mat_vec; which_is_unsatisfied agrees with ark355_is_satisfied before and after a planted violation."""
    C, lib, ctx = BLS12_381, gpu_lib, gpu_ctx
    p, n = C.r, 1 << 18
    ell, w, mats, z = bench_lc_shape(p, n)
    m = ell + w
    r1 = lib.r1cs_load(ctx, C.curve_id, n, ell, w, mats)
    s = SR1CS.from_r1cs(lib, ctx, r1, C.curve_id, m)
    try:
        n_ell, n_w, rows, nnz = s.dims
        P = n_ell - 1
        used = set(np.unique(np.concatenate([mat[1] for mat in mats])).tolist()) - {0}
        assert P == 1 and rows == 2 * n + P and n_w == len(used) + n   # x is used: one input; every used column a witness
        assert nnz == (2 * (len(mats[0][1]) + len(mats[1][1])) + 2, 3 * n)
        zb = bytearray(S._mont_bytes(p, z))
        fr = lambda b, i: int.from_bytes(b[32 * i:32 * i + 32], "little") * pow(1 << 256, -1, p) % p      # noqa: E731
        rnd = random.Random(0x18)
        sample = sorted(set(rnd.sample(range(n), 4094)) | {0, n - 1})
        bad = n - 77                                                   # the fresh witness of this row: C of the row
        for planted in (False, True):
            if planted:
                zb[32 * (12 + bad):32 * (13 + bad)] = S._mont_bytes(p, [(z[12 + bad] + 1) % p])
            first = lib.is_satisfied(ctx, r1, zb, m)
            assert first == (bad if planted else -1)
            zp = s.assignment(zb)
            assert s.system.which_is_unsatisfied(zp) == ((sc.SR1CS_LABEL, 2 * bad) if planted else None)
            az, bz, cz = lib.mat_vec(ctx, r1, zb, m, n, 32)
            m0, m1 = s.system.mat_vec(sc.SR1CS_LABEL, zp)
            for i in sample + [bad]:
                a, b, c = fr(az, i), fr(bz, i), fr(cz, i)
                sq = (a - b) ** 2 % p
                assert fr(m0, 2 * i) == (a + b) % p and fr(m0, 2 * i + 1) == (a - b) % p, i
                assert fr(m1, 2 * i) == (4 * c + sq) % p and fr(m1, 2 * i + 1) == sq, i
            assert fr(m0, 2 * n) == 0 and m1[32 * 2 * n:] == bytes(32)                     # the equality row
    finally:
        s.free()
        lib.dll.ark355_r1cs_free(r1)
