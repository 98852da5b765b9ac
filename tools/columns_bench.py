#!/usr/bin/env python3
"""Column-polynomial micro-benchmark: ark355_gr1cs_columns_at_dev against the generator's own scalar stages, both curves.
  (a) ark355_gr1cs_columns_at_dev on the R1CS shape of the 2^20-row mul-chain bench circuit plus its ell instance rows (A row
      n + i = e_i, B and C empty), the output in device memory;
  (b) ark355_setup asked for u, v, w only, on the same instance in the same process: the same three stages (Lagrange vector,
      column-major order, gather) from the SAME kernels (colgather_impl.cuh serves both), plus the combination kernel, the
      canonical conversion, per-call allocations and three copies back -- what the resident scratch of (a) saves, not a
      yardstick for the kernels;
  (c) the SR1CS system of that circuit (2 n + P rows, t = 2);
  (d) a degree-3 predicate of arity 4 at 2^18 rows.
(c) and (d) are first measurements with nothing to compare against.  The readings are interleaved after a warm-up of every call;
each line gives the median, the minimum and the spread over the repeats.  Host-clock times of synchronous calls (each returns
after a stream synchronise).  The box's multiply-add rate (ark355_diag_mad_rate) is read before and after.  Kernel times come
from a `rocprofv3 --kernel-trace --stats` run of this script of its own.  Dev tool; run on an MI355X:
  python tools/columns_bench.py [--log-n 20] [--reps 20] [--out profiles/columns_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np

import snark_amd
from snark_amd import GR1CS, params, synthetic
from quotient_bench import degree3_predicate, r1cs_predicate

TAU = 987654321


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-n3", type=int, default=18, help="log2 of the rows of the degree-3 predicate")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--cases", default="a,b,c,d", help="which of the four calls to time (a traced run splits its kernels by case)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "columns_bench measures on the GPU: there is nothing to report without one"
    n = 1 << a.log_n
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def dev(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    say("columns_bench: mul-chain, n = 2^%d rows, %d interleaved repeats after %d warm-up rounds; ms per call (host clock around "
        "synchronous calls); COLS_LANE_MAX = %d" % (a.log_n, a.reps, a.warmup, lib.ctx_get_policy(ctx, "COLS_LANE_MAX")))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    tau = TAU.to_bytes(32, "little")
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        sizes = lib.sizes(cv.curve_id)
        r1, _ = synthetic.mulchain(cv, n)
        ell, w = r1.ell, r1.w
        m = ell + w
        h_r1 = lib.r1cs_load(ctx, cv.curve_id, n, ell, w, list(zip(r1.row_ptr, r1.col, r1.coeff)))
        N = lib.dll.ark355_r1cs_domain_size(h_r1)
        td = b"".join(cv.fr_canon(x) for x in (TAU, 5, 7, 11, 13))
        # (a)
        ga = GR1CS(cv, ell, w, [r1cs_predicate(cv, r1)]).load(lib, ctx)
        d_a = dev(3 * m * 32)
        # (c)
        s = lib.sr1cs_from_r1cs(ctx, h_r1)
        ell2, w2, rows, _ = lib.sr1cs_dims(s)
        sysc = lib.sr1cs_system(s)
        d_c = dev(2 * (ell2 + w2) * 32)
        # (d)
        n3, m3 = 1 << a.log_n3, 64
        g3 = GR1CS(cv, 1, m3 - 1, [degree3_predicate(cv, n3, m3)]).load(lib, ctx)
        d_d = dev(4 * m3 * 32)
        torch.cuda.synchronize()
        vp = lambda t: t.data_ptr()                            # noqa: E731

        def call_a():
            ga.columns_at_dev("R1CS", TAU, vp(d_a))

        def call_b():
            return lib.setup(ctx, h_r1, cv.g1_gen_raw(), cv.g2_gen_raw(), td, (ell, w, N), sizes, want=("u", "v", "w"), want_pk=False)[0]

        def call_c():
            lib.gr1cs_columns_at_dev(ctx, sysc, 0, tau, 0, vp(d_c))

        def call_d():
            g3.columns_at_dev("deg3", TAU, vp(d_d))

        calls = [("(a) ark355_gr1cs_columns_at_dev, R1CS shape", call_a), ("(b) ark355_setup, u v w only", call_b),
                 ("(c) ark355_gr1cs_columns_at_dev, SR1CS system", call_c), ("(d) ark355_gr1cs_columns_at_dev, degree 3", call_d)]
        calls = [c for c in calls if c[0][1] in a.cases.split(",")]
        # the two routes compute the same values: (a) Montgomery, (b) canonical
        uvw = call_b()
        call_a()
        got = np.frombuffer(d_a.cpu().numpy().tobytes(), dtype=np.uint8).reshape(3, m, 32)
        rinv = pow(1 << 256, -1, cv.r)
        for k, key in enumerate(("u", "v", "w")):
            want = uvw[key].reshape(m, 32)
            for j in list(range(8)) + list(range(m - 8, m)) + [m // 2, m // 3]:
                assert int.from_bytes(got[k][j].tobytes(), "little") * rinv % cv.r == int.from_bytes(want[j].tobytes(), "little"), (key, j)
        for _ in range(a.warmup):
            for _, f in calls:
                f()
        t = [[] for _ in calls]
        for _ in range(a.reps):
            for k, (_, f) in enumerate(calls):
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        say("%s: (a) (b) %d rows, N = 2^%d, m = %d; (c) %d rows, m = %d; (d) %d rows, arity 4, m = %d"
            % (name, n + ell, N.bit_length() - 1, m, rows, ell2 + w2, n3, m3))
        med = []
        for (label, _), ts in zip(calls, t):
            q = statistics.quantiles(ts, n=4)
            med.append(statistics.median(ts))
            say("  %-52s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, med[-1], min(ts), max(ts) - min(ts), q[2] - q[0]))
        if a.cases.startswith("a,b"):
            say("  (a) / (b) = %.3f" % (med[0] / med[1]))
        g3.free()
        lib.sr1cs_free(s)
        ga.free()
        lib.dll.ark355_r1cs_free(h_r1)
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
