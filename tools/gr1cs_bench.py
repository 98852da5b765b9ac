#!/usr/bin/env python3
"""GR1CS micro-benchmark: the fused satisfaction check and the general mat-vec against the R1CS-only entries, at 2^20 rows,
on resident handles and an assignment in page-locked host memory (every entry copies z to the device: 32 MiB, the same for
both sides of each comparison).
  (a) ark355_is_satisfied                on the mul-chain R1CS (SpMV writing three vectors + the check kernel reading them)
  (b) ark355_gr1cs_which_is_unsatisfied  on the same matrices loaded as one predicate (one fused kernel, no vector written)
  (c) ark355_gr1cs_which_is_unsatisfied  on the three-predicate system of tests/test_gpu_gr1cs.py (R1CS, x0^5 + x1 x2 - x3, SR1CS)
  (d) ark355_r1cs_mat_vec against ark355_gr1cs_mat_vec on (a)'s matrices (both copy 3 x 32 MiB back)
The readings are interleaved (a, b, c, d, d', a, b, ...) after a warm-up of every call; each line gives the median, the
minimum and the spread (max - min, and the interquartile range) over the repeats.  The spread of (a) is the noise figure
(b) is held against.  Algorithmic bytes of a check = CSR entries (column + coefficient index + the gathered 32-byte z
element) + row pointers.  Host-clock times of synchronous calls; kernel times come from a `rocprofv3 --kernel-trace --stats`
run of this script (kernels gr1cs_pred_kernel, gr1cs_spmv_kernel, r1cs_spmv_kernel, r1cs_check_kernel).
Dev tool; run on an MI355X:  python tools/gr1cs_bench.py [--log-n 20] [--reps 30] [--out profiles/gr1cs_microbench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import snark_amd
from snark_amd import GR1CS, params, synthetic
from snark_amd.gr1cs import Predicate


def pinned(lib, data: bytes):
    p = C.c_void_p()
    rc = lib.dll.ark355_host_alloc(len(data), C.byref(p))
    assert rc == 0, rc
    C.memmove(p, data, len(data))
    return np.ctypeslib.as_array((C.c_uint8 * len(data)).from_address(p.value)), p


def check_bytes(preds):
    return sum(int(rp[-1]) * (4 + 4 + 32) + rp.size * 4 for p in preds for rp in p.row_ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gr1cs_cases as gc
    from oracle.fields import BLS12_381 as OC
    cv = params.BLS12_381
    n = 1 << a.log_n
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    r1, z = synthetic.mulchain(cv, n)
    m = r1.ell + r1.w
    zb, zp = pinned(lib, synthetic.z_to_mont_bytes(cv, z))
    h_r1 = lib.r1cs_load(ctx, cv.curve_id, n, r1.ell, r1.w, list(zip(r1.row_ptr, r1.col, r1.coeff)))
    one = GR1CS(cv, r1.ell, r1.w, [Predicate("R1CS", 3, gc.r1cs_terms(cv.r), n, list(r1.row_ptr), list(r1.col), list(r1.coeff))])
    one.load(lib, ctx)
    s = gc.ScaleSystem(OC, n)
    three = s.gr1cs().load(lib, ctx)
    zb3, zp3 = pinned(lib, synthetic.z_to_mont_bytes(cv, s.z))
    out3 = np.zeros(3 * n * 32, dtype=np.uint8)
    o = [out3[i * n * 32:(i + 1) * n * 32].ctypes.data_as(C.c_void_p) for i in range(3)]

    def call_a():
        assert lib.is_satisfied(ctx, h_r1, zb, m) == -1

    def call_b():
        assert lib.gr1cs_which_is_unsatisfied(ctx, one.handle, zb, m) is None

    def call_c():
        assert lib.gr1cs_which_is_unsatisfied(ctx, three.handle, zb3, three.m) is None

    def call_d_r1cs():
        lib.check(ctx, lib.dll.ark355_r1cs_mat_vec(ctx, h_r1, zb.ctypes.data_as(C.c_void_p), m, *o))

    def call_d_gr1cs():
        lib.check(ctx, lib.dll.ark355_gr1cs_mat_vec(ctx, one.handle, 0, zb.ctypes.data_as(C.c_void_p), m, out3.ctypes.data_as(C.c_void_p)))

    calls = [("(a) ark355_is_satisfied, mul-chain R1CS", call_a, check_bytes(one.predicates)),
             ("(b) ark355_gr1cs_which_is_unsatisfied, same matrices, one predicate", call_b, check_bytes(one.predicates)),
             ("(c) ark355_gr1cs_which_is_unsatisfied, three predicates", call_c, check_bytes(three.predicates)),
             ("(d) ark355_r1cs_mat_vec", call_d_r1cs, check_bytes(one.predicates)),
             ("(d') ark355_gr1cs_mat_vec, same matrices", call_d_gr1cs, check_bytes(one.predicates))]
    call_d_r1cs()
    ref = out3.copy()
    call_d_gr1cs()
    assert np.array_equal(ref, out3), "the two mat-vec entries disagree"
    for _ in range(a.warmup):
        for _, f, _ in calls:
            f()
    t = [[] for _ in calls]
    for _ in range(a.reps):
        for k, (_, f, _) in enumerate(calls):
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    say("gr1cs_bench: n = 2^%d rows, BLS12-381 Fr, %d interleaved repeats after %d warm-up rounds; ms per call (host clock, "
        "z copied from page-locked memory inside every call)" % (a.log_n, a.reps, a.warmup))
    for (name, _, nbytes), ts in zip(calls, t):
        q = statistics.quantiles(ts, n=4)
        med = statistics.median(ts)
        say("%-70s median %7.3f  min %7.3f  max-min %6.3f  iqr %6.3f   algorithmic %6.1f MB -> %6.1f GB/s at the median"
            % (name, med, min(ts), max(ts) - min(ts), q[2] - q[0], nbytes / 1e6, nbytes / med / 1e6))
    med = [statistics.median(x) for x in t]
    say("(b) - (a) = %+.3f ms at the median; spread of (a): max-min %.3f ms, iqr %.3f ms"
        % (med[1] - med[0], max(t[0]) - min(t[0]), statistics.quantiles(t[0], n=4)[2] - statistics.quantiles(t[0], n=4)[0]))
    say("(d') - (d) = %+.3f ms at the median; spread of (d): max-min %.3f ms"
        % (med[4] - med[3], max(t[3]) - min(t[3])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    one.free()
    three.free()
    lib.dll.ark355_r1cs_free(h_r1)
    lib.dll.ark355_host_free(zp)
    lib.dll.ark355_host_free(zp3)
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
