#!/usr/bin/env python3
"""Micro-benchmark of the batched short MSMs (ark355_msm_batch_dev).  Three measurements, each from one
process, interleaved after a warm-up of every call, `--reps` repeats (default 8); every line gives the median and max - min:
  crossover      per n = 2^0 .. 2^14, ONE segment against a handle of exactly n bases, both curves and groups: the short route
                 (MSM_BATCH_SMALL_MAX = 2^14) against ark355_msm_dev.  The last line names the largest power of two at which the
                 short route wins by more than the two spreads combined on every curve and group measured: the shipped default of
                 MSM_BATCH_SMALL_MAX follows from it.
  opening        ark355_mle_open_dev at N = 2^18 and 2^22 (G1) under MSM_BATCH_SMALL_MAX = 0 and under the default, alternating.
  batch scaling  64 segments of 1024 scalars in one call against 64 calls of ark355_msm_dev.
The bases are multiples of the generator by the scalars themselves: any points do for timing.  Host-clock times of synchronous calls
(each returns after a stream synchronise); kernel times proper need a `rocprofv3 --kernel-trace --stats` run of this script of its
own.  Dev tool; run on an MI355X:
  python tools/msm_batch_bench.py [--parts crossover,opening,scaling] [--open-logs 18,22] [--reps 8] [--out profiles/msm_batch_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

import numpy as np

import snark_amd
from snark_amd import params

LIMIT = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="crossover,opening,scaling")
    ap.add_argument("--open-logs", default="18,22")
    ap.add_argument("--max-log", type=int, default=LIMIT)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "msm_batch_bench measures on the GPU: there is nothing to report without one"
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def med_spread(ts):
        return statistics.median(ts), max(ts) - min(ts)

    parts = a.parts.split(",")
    groups = [int(g) for g in a.groups.split(",")]
    default = lib.ctx_get_policy(ctx, "MSM_BATCH_SMALL_MAX")
    say("msm_batch_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock around synchronous calls); median (max - min)"
        % (a.reps, a.warmup))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    rng = np.random.default_rng(0x0B47)
    pb = lambda pt: b"".join(int(x).to_bytes(32, "little") for x in pt)   # noqa: E731
    wins = {}
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        p, cid = cv.r, cv.curve_id
        top = (1 << ((p >> 248).bit_length() - 1)) - 1         # words below r: valid scalars
        big = 1 << max(a.max_log, 10)
        words = rng.integers(0, 256, size=(64 * 1024 if "scaling" in parts else big, 32), dtype=np.uint8)
        words[:, 31] &= top
        d_s = torch.from_numpy(words).cuda().reshape(-1)
        torch.cuda.synchronize()
        for group in groups:
            size = lib.sizes(cid)["g1" if group == 1 else "g2"]
            gen = cv.g1_gen_raw() if group == 1 else cv.g2_gen_raw()
            pts = lib.fixed_base_mul_dev(ctx, cid, group, gen, d_s.data_ptr(), big, False, size)
            if "crossover" in parts:
                say("crossover, %s G%d: one segment of n scalars against a handle of n bases" % (name, group))
                for lg in range(a.max_log + 1):
                    n = 1 << lg
                    h = lib.bases_load(ctx, cid, group, pts[:n * size], n)
                    T = {"short": [], "msm_dev": []}
                    want = None
                    for rep in range(a.warmup + a.reps):
                        lib.ctx_set_policy(ctx, "MSM_BATCH_SMALL_MAX", 1 << LIMIT)
                        t0 = time.perf_counter()
                        got = lib.msm_batch_dev(ctx, [h], [d_s.data_ptr()], [n], 0, size)
                        t1 = time.perf_counter()
                        ref = lib.msm_dev(ctx, h, d_s.data_ptr(), n, 0, size)
                        t2 = time.perf_counter()
                        want = want or ref
                        assert got == ref == want, "the two routes disagree"
                        if rep >= a.warmup:
                            T["short"].append((t1 - t0) * 1e3)
                            T["msm_dev"].append((t2 - t1) * 1e3)
                    (ms, ss), (mm, sm) = med_spread(T["short"]), med_spread(T["msm_dev"])
                    win = ms + ss + sm < mm
                    wins.setdefault(lg, []).append(win)
                    say("  n = 2^%-2d  short %8.3f (%6.3f)   msm_dev %8.3f (%6.3f)   %s" % (lg, ms, ss, mm, sm, "short wins" if win else "-"))
                    lib.dll.ark355_bases_free(h)
                flush()
            if "scaling" in parts:
                h = lib.bases_load(ctx, cid, group, pts[:1024 * size], 1024)
                ptrs = [d_s.data_ptr() + 32 * 1024 * i for i in range(64)]
                T = {"one batch of 64 x 1024 (short route)": [], "one batch of 64 x 1024 (MSM_BATCH_SMALL_MAX = 0)": [], "64 calls of msm_dev": []}
                for rep in range(a.warmup + a.reps):
                    lib.ctx_set_policy(ctx, "MSM_BATCH_SMALL_MAX", 1024)
                    t0 = time.perf_counter()
                    got = lib.msm_batch_dev(ctx, [h] * 64, ptrs, [1024] * 64, 0, size)
                    t1 = time.perf_counter()
                    lib.ctx_set_policy(ctx, "MSM_BATCH_SMALL_MAX", 0)
                    off = lib.msm_batch_dev(ctx, [h] * 64, ptrs, [1024] * 64, 0, size)
                    t2 = time.perf_counter()
                    ref = b"".join(lib.msm_dev(ctx, h, q, 1024, 0, size) for q in ptrs)
                    t3 = time.perf_counter()
                    assert got == off == ref, "the routes disagree"
                    if rep >= a.warmup:
                        for k, dt in zip(T, (t1 - t0, t2 - t1, t3 - t2)):
                            T[k].append(dt * 1e3)
                say("batch scaling, %s G%d:" % (name, group))
                for k, ts in T.items():
                    say("  %-52s %9.3f (%6.3f)" % ((k,) + med_spread(ts)))
                lib.dll.ark355_bases_free(h)
                flush()
        if "opening" in parts:
            size = lib.sizes(cid)["g1"]
            for v in (int(x) for x in a.open_logs.split(",") if x):
                N = 1 << v
                w2 = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
                w2[:, 31] &= top
                d_f = torch.from_numpy(w2).cuda().reshape(-1)
                point = [int.from_bytes(rng.bytes(31), "little") for _ in range(v)]
                t0 = time.perf_counter()
                pts2 = lib.fixed_base_mul_dev(ctx, cid, 1, cv.g1_gen_raw(), d_f.data_ptr(), N // 2, True, size)
                handles = [lib.bases_load(ctx, cid, 1, pts2[:(N >> (j + 1)) * size], N >> (j + 1)) for j in range(v)]
                say("opening, %s G1, N = 2^%d (handles of 2^%d .. 1 points built in %.1f s)" % (name, v, v - 1, time.perf_counter() - t0))
                T = {"open_dev, MSM_BATCH_SMALL_MAX = 0": [], "open_dev, default (%d)" % default: []}
                want = None
                for rep in range(a.warmup + a.reps):
                    ts = []
                    for value in (0, default):
                        lib.ctx_set_policy(ctx, "MSM_BATCH_SMALL_MAX", value)
                        t0 = time.perf_counter()
                        got = lib.mle_open_dev(ctx, cid, handles, d_f.data_ptr(), v, pb(point), size)
                        ts.append(time.perf_counter() - t0)
                        want = want or got
                        assert got == want, "the opening depends on the policy"
                    if rep >= a.warmup:
                        for k, dt in zip(T, ts):
                            T[k].append(dt * 1e3)
                for k, ts in T.items():
                    say("  %-52s %9.3f (%6.3f)" % ((k,) + med_spread(ts)))
                for h in handles:
                    lib.dll.ark355_bases_free(h)
                del d_f
                flush()
    lib.ctx_set_policy(ctx, "MSM_BATCH_SMALL_MAX", default)
    if wins:
        best = [lg for lg in sorted(wins) if all(wins[lg])]
        say("crossover: the short route wins by more than both spreads on every curve and group measured at n = %s"
            % (", ".join("2^%d" % lg for lg in best) or "no length"))
        say("crossover: largest such power of two: %s" % ("2^%d" % best[-1] if best else "none -- the default would be 0"))
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    flush()
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
