#!/usr/bin/env python3
"""Square R1CS micro-benchmark: the device adapter on the 2^20-constraint mul-chain bench circuit, both curves.
  (a) ark355_sr1cs_from_r1cs        once per circuit: numbering, fill, pool, the copies of A and B (handle freed after each call)
  (b) ark355_sr1cs_assignment_dev   once per proof: z and z' in device memory (two launches and a stream synchronise)
  (c) ark355_r1cs_mat_vec           on the same r1cs handle, outputs NULL: z copied from page-locked host memory, the SpMV of
                                    A, B, C into three resident vectors, nothing copied back -- the path every proof already runs
  (d) the host-to-device copy of z alone (torch, the same page-locked buffer): what (c) carries and (b) does not
The readings are interleaved (a, b, c, d, a, ...) after a warm-up of every call; each line gives the median, the minimum and the
spread over the repeats.  Host-clock times of synchronous calls.  The expectation under test: the assignment pass costs no more
than the mat-vec -- two of its three row dots, one vector and a scatter written against three vectors.  Like for like that is
(b) against (c) - (d), and, free of launch and synchronise overheads, the kernel times of a `rocprofv3 --kernel-trace --stats`
run of this script (--reps 5): sr1cs_assign_kernel + sr1cs_scatter_kernel against r1cs_spmv_kernel.
Dev tool; run on an MI355X:  python tools/sr1cs_bench.py [--log-n 20] [--reps 20] [--out profiles/sr1cs_bench.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np

import snark_amd
from snark_amd import params, synthetic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "sr1cs_bench measures on the GPU: there is nothing to report without one"
    n = 1 << a.log_n
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("sr1cs_bench: mul-chain, n = 2^%d rows, %d interleaved repeats after %d warm-up rounds; ms per call (host clock)"
        % (a.log_n, a.reps, a.warmup))
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        r1, z = synthetic.mulchain(cv, n)
        m = r1.ell + r1.w
        h_r1 = lib.r1cs_load(ctx, cv.curve_id, n, r1.ell, r1.w, list(zip(r1.row_ptr, r1.col, r1.coeff)))
        z_host = torch.from_numpy(np.frombuffer(synthetic.z_to_mont_bytes(cv, z), dtype=np.uint8).copy()).pin_memory()
        d_z = z_host.cuda()
        s = lib.sr1cs_from_r1cs(ctx, h_r1)
        ell2, w2, rows, nnz = lib.sr1cs_dims(s)
        d_out = torch.zeros((ell2 + w2) * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        null = C.c_void_p(None)

        def call_a():
            lib.sr1cs_free(lib.sr1cs_from_r1cs(ctx, h_r1))

        def call_b():
            lib.sr1cs_assignment_dev(ctx, s, d_z.data_ptr(), m, d_out.data_ptr())

        def call_c():
            lib.check(ctx, lib.dll.ark355_r1cs_mat_vec(ctx, h_r1, C.c_void_p(z_host.data_ptr()), m, null, null, null))

        def call_d():
            d_z.copy_(z_host, non_blocking=True)
            torch.cuda.synchronize()

        calls = [("(a) ark355_sr1cs_from_r1cs (+ free)", call_a), ("(b) ark355_sr1cs_assignment_dev", call_b),
                 ("(c) ark355_r1cs_mat_vec, pinned z, no copy back", call_c), ("(d) copy of z to the device alone", call_d)]
        # the pass computes what the existing entries compute: z' satisfies the system exactly when z satisfies the R1CS
        call_b()
        zp = d_out.cpu().numpy().tobytes()
        assert lib.is_satisfied(ctx, h_r1, z_host.numpy(), m) == -1
        assert lib.gr1cs_which_is_unsatisfied(ctx, lib.sr1cs_system(s), zp, ell2 + w2) is None
        for _ in range(a.warmup):
            for _, f in calls:
                f()
        t = [[] for _ in calls]
        for _ in range(a.reps):
            for k, (_, f) in enumerate(calls):
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        say("%s: R1CS %d rows, %d variables, nnz %s  ->  SR1CS %d rows, %d + %d variables, nnz %s"
            % (name, n, m, [int(x[-1]) for x in r1.row_ptr], rows, ell2, w2, list(nnz)))
        med = []
        for (label, _), ts in zip(calls, t):
            q = statistics.quantiles(ts, n=4)
            med.append(statistics.median(ts))
            say("  %-52s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, med[-1], min(ts), max(ts) - min(ts), q[2] - q[0]))
        say("  (b) = %.3f ms; (c) - (d) = %.3f ms, a difference of two host-clock medians with a synchronise in each: the spreads "
            "above are its noise, and the kernel times of the traced run decide between the two" % (med[1], med[2] - med[3]))
        lib.sr1cs_free(s)
        lib.dll.ark355_r1cs_free(h_r1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
