#!/usr/bin/env python3
"""Micro-benchmark of the multilinear openings: ark355_mle_quotients_fr_dev and ark355_mle_open_dev at N = 2^18 and 2^22 entries,
both curves, one table and four.
Per shape, from one run, interleaved after a warm-up of every call:
  quotients_dev, E = 1, 2, 4, 8   the quotient tables under MLE_OPEN_LANE_ENTRIES = E: ceil(v / log2(256 E)) launches, the table read
                                  once, count N Fr written
  (i)                             a device-to-device copy of the tables, count N Fr: the traffic floor (one read, one write)
  (ii)                            ark355_mle_eval_fr_dev on the same tables: v launches that store no quotient
and for one table (--open-logs):
  open_dev                        the quotients and the v MSMs against resident G1 handles
  v x msm_dev                     the same v ark355_msm_dev calls on the rows of a quotients_dev output computed beforehand, their sum,
                                  and the part of it spent on the levels of at most 2^10 scalars, which is per-call overhead
The handles hold multiples of the generator by the table's own entries: any points do for timing.  Each line gives the median, the
minimum and the spread over the repeats.  Host-clock times of synchronous calls (each returns after a stream synchronise); kernel
times proper need a `rocprofv3 --kernel-trace --stats` run of this script of its own.  The box's multiply-add rate
(ark355_diag_mad_rate) is read before and after.  Dev tool; run on an MI355X:
  python tools/mle_open_bench.py [--logs 18,22] [--open-logs 18,22] [--reps 10] [--out profiles/mle_open_bench.txt]"""
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
from snark_amd.poly import Mle

SMALL = 10                                                     # levels of at most 2^SMALL scalars count as "small"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="18,22")
    ap.add_argument("--open-logs", default="18,22")
    ap.add_argument("--counts", default="1,4")
    ap.add_argument("--entries", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "mle_open_bench measures on the GPU: there is nothing to report without one"
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def dev(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def stat(label, ts):
        q = statistics.quantiles(ts, n=4) if len(ts) > 1 else [ts[0]] * 3
        say("  %-52s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, statistics.median(ts), min(ts), max(ts) - min(ts), q[2] - q[0]))
        return statistics.median(ts)

    say("mle_open_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock around synchronous calls)" % (a.reps, a.warmup))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    rng = np.random.default_rng(0x0BE4)
    vp = lambda t: t.data_ptr()                                # noqa: E731
    pb = lambda pt: b"".join(int(x).to_bytes(32, "little") for x in pt)   # noqa: E731
    entries = [int(x) for x in a.entries.split(",")]
    open_logs = [int(x) for x in a.open_logs.split(",") if x]
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        p, cid = cv.r, cv.curve_id
        top = (1 << ((p >> 248).bit_length() - 1)) - 1         # words below r: valid Montgomery images
        for v in (int(x) for x in a.logs.split(",")):
            N = 1 << v
            point = [int.from_bytes(rng.bytes(31), "little") for _ in range(v)]
            for count in (int(x) for x in a.counts.split(",")):
                words = rng.integers(0, 256, size=(count * N, 32), dtype=np.uint8)
                words[:, 31] &= top
                d_f = torch.from_numpy(words).cuda().reshape(-1)
                d_q, d_copy, d_rem, d_val = dev(count * N * 32), dev(count * N * 32), dev(count * 32), dev(count * 32)
                torch.cuda.synchronize()
                say("%s, N = 2^%d, %d table%s: %d MiB in, %d MiB out" % (name, v, count, "s" if count > 1 else "", count * N * 32 >> 20, count * N * 32 >> 20))
                keys = ["quotients_dev, E = %d" % E for E in entries] + ["(i) device-to-device copy of the tables", "(ii) mle_eval_fr_dev"]
                T = {k: [] for k in keys}
                for rep in range(a.warmup + a.reps):
                    ts = []
                    for E in entries:
                        lib.ctx_set_policy(ctx, "MLE_OPEN_LANE_ENTRIES", E)
                        t0 = time.perf_counter()
                        lib.mle_quotients_fr_dev(ctx, cid, vp(d_f), v, count, pb(point), vp(d_q), vp(d_rem))
                        ts.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    d_copy.copy_(d_f)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    lib.mle_eval_fr_dev(ctx, cid, vp(d_f), v, count, pb(point), vp(d_val))
                    t2 = time.perf_counter()
                    ts += [t1 - t0, t2 - t1]
                    if rep >= a.warmup:
                        for k, dt in zip(keys, ts):
                            T[k].append(dt * 1e3)
                lib.ctx_set_policy(ctx, "MLE_OPEN_LANE_ENTRIES", 0)
                assert bytes(d_rem.cpu().numpy()) == bytes(d_val.cpu().numpy()), "the values of the two routes differ"
                med = {k: stat(k, ts) for k, ts in T.items()}
                d8 = med.get("quotients_dev, E = 8", med[keys[0]])
                say("  quotients_dev at the default / copy = %.2f, / eval = %.2f; best E = %d"
                    % (d8 / med[keys[-2]], d8 / med[keys[-1]], min(entries, key=lambda E: med["quotients_dev, E = %d" % E])))
                if count == 1 and v in open_logs:
                    size = lib.sizes(cid)["g1"]
                    t0 = time.perf_counter()
                    pts = lib.fixed_base_mul_dev(ctx, cid, 1, cv.g1_gen_raw(), vp(d_f), N // 2, True, size)
                    handles = [lib.bases_load(ctx, cid, 1, pts[:(N >> (j + 1)) * size], N >> (j + 1)) for j in range(v)]
                    say("  (handles of 2^%d .. 1 points built in %.1f s)" % (v - 1, time.perf_counter() - t0))
                    lib.mle_quotients_fr_dev(ctx, cid, vp(d_f), v, 1, pb(point), vp(d_q), vp(d_rem))
                    T = {"open_dev": [], "v x msm_dev on precomputed rows, sum": [], "  of which levels of <= 2^%d scalars (%d calls)" % (SMALL, min(v, SMALL + 1)): []}
                    per_level = [[] for _ in range(v)]
                    want = None
                    for rep in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        got = lib.mle_open_dev(ctx, cid, handles, vp(d_f), v, pb(point), size)
                        t1 = time.perf_counter()
                        rows = b""
                        lv = []
                        for j in range(v):
                            off, ln = Mle.level(v, j)
                            u0 = time.perf_counter()
                            rows += lib.msm_dev(ctx, handles[j], vp(d_q) + off * 32, ln, 1, size)
                            lv.append(time.perf_counter() - u0)
                        want = want or got
                        assert got == want and got[0] == rows, "open_dev and the v msm_dev calls disagree"
                        if rep >= a.warmup:
                            for k, dt in zip(T, (t1 - t0, sum(lv), sum(lv[j] for j in range(v) if v - 1 - j <= SMALL))):
                                T[k].append(dt * 1e3)
                            for j in range(v):
                                per_level[j].append(lv[j] * 1e3)
                    m = [stat(k, ts) for k, ts in T.items()]
                    say("  open_dev / sum of the MSMs = %.3f; small levels = %.0f %% of the MSM time" % (m[0] / m[1], 100.0 * m[2] / m[1]))
                    say("  msm_dev per level, median ms: " + " ".join("%d:%.2f" % (v - 1 - j, statistics.median(per_level[j])) for j in range(v)) + "  (log2 scalars : ms)")
                    for h in handles:
                        lib.dll.ark355_bases_free(h)
                del d_f, d_q, d_copy
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
