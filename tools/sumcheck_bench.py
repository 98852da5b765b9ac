#!/usr/bin/env python3
"""Micro-benchmark of the multilinear side: the sum-check of a predicate over resident tables (ark355_gr1cs_sumcheck_begin_dev,
ark355_sumcheck_round, ark355_sumcheck_finish) and the primitives ark355_mle_eq_fr_dev, ark355_mle_fix_fr_dev (k = 1) and
ark355_mle_eval_fr_dev, at N = 2^22 and 2^18 entries, the R1CS (x0 x1 - x2) and SR1CS (x0^2 - x1) shapes with the weight eq(tau),
both curves.  The tables are what ark355_gr1cs_mat_vec_dev leaves for a system of one-entry rows and a random assignment.
Per shape, from one run, interleaved after a warm-up of every call:
  round 1                 ark355_sumcheck_round(NULL): the kernel over the caller's tables, the reduction, one 32 * points byte copy
                          back and the host wait
  round 2 (fused)         ark355_sumcheck_round(r_1): fold and sum in one kernel
  rounds 3 .. v + finish  the rest of the run, and the wall time of the whole run with its v + 1 host round trips (begin excluded;
                          it allocates and is listed on its own)
  unfused round 2         ark355_mle_fix_fr_dev (k = 1) of the t + 1 tables, then round 1 of a run begun on the result: the route the
                          fused kernel has to beat
  (i)                     a device-to-device copy of the bytes round 1 reads, (t + 1) N Fr: the traffic floor
  (ii)                    ark355_gr1cs_quotient_dev on the same system and assignment, for context
  eq, fix (k = 1), eval   alone on one table of N entries, next to a copy of N Fr
under SUMCHECK_LANE_PAIRS = 1, 2, 4, 8 (--pairs).  Each line gives the median, the minimum and the spread over the repeats.
Host-clock times of synchronous calls (each returns after a stream synchronise), so a round includes one launch-and-wait
latency; kernel times proper need a `rocprofv3 --kernel-trace --stats` run of this script of its own.  The box's multiply-add
rate (ark355_diag_mad_rate) is read before and after.  Dev tool; run on an MI355X:
  python tools/sumcheck_bench.py [--logs 22,18] [--reps 10] [--out profiles/sumcheck_bench.txt]"""
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
from snark_amd.gr1cs import Predicate

M = 64                                                         # variables of the assignment


def one_entry_predicate(cv, label, arity, terms, n):
    """entry (1, 1 + (i (k + 3)) mod (M - 1)) in row i of matrix k"""
    i = np.arange(n, dtype=np.int64)
    rp = np.arange(n + 1, dtype=np.uint64)
    one = np.frombuffer(cv.fr_mont(1), dtype=np.uint8)
    cols = [(1 + (i * (k + 3)) % (M - 1)).astype(np.uint32) for k in range(arity)]
    return Predicate(label, arity, terms, n, [rp] * arity, cols, [np.tile(one, n).tobytes()] * arity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="22,18")
    ap.add_argument("--pairs", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "sumcheck_bench measures on the GPU: there is nothing to report without one"
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

    say("sumcheck_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock around synchronous calls)" % (a.reps, a.warmup))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    rng = np.random.default_rng(0x5C)
    vp = lambda t: t.data_ptr()                                # noqa: E731
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        p, cid = cv.r, cv.curve_id
        z = [1] + [int.from_bytes(rng.bytes(31), "little") for _ in range(M - 1)]
        d_z = torch.from_numpy(np.frombuffer(synthetic.z_to_mont_bytes(cv, z), dtype=np.uint8).copy()).cuda()
        shapes = [("R1CS", 3, [(1, [(0, 1), (1, 1)]), (p - 1, [(2, 1)])]), ("SR1CS", 2, [(1, [(0, 2)]), (p - 1, [(1, 1)])])]
        for v in (int(x) for x in a.logs.split(",")):
            N = 1 << v
            tau = [int.from_bytes(rng.bytes(31), "little") for _ in range(v)]
            ch = [int.from_bytes(rng.bytes(31), "little") for _ in range(v)]
            pb = lambda pt: b"".join(int(x).to_bytes(32, "little") for x in pt)   # noqa: E731
            d_w = dev(N * 32)
            d_one, d_half, d_val = dev(N * 32), dev(N * 16), dev(32)
            for label, t, terms in shapes:
                g = GR1CS(cv, 1, M - 1, [one_entry_predicate(cv, label, t, terms, N)]).load(lib, ctx)
                d_t = dev(t * N * 32)
                g.mat_vec_dev(label, vp(d_z), M, vp(d_t))
                lib.mle_eq_fr_dev(ctx, cid, v, pb(tau), vp(d_w))
                d_all = torch.cat([d_t, d_w])                  # t + 1 tables back to back: the unfused route folds them in one call
                d_fold = dev((t + 1) * (N // 2) * 32)
                d_copy = dev((t + 1) * N * 32)
                d_h = dev(g.quotient_dims(label)[3] * 32)
                torch.cuda.synchronize()
                say("%s, %s with a weight, N = 2^%d: round 1 reads %d MiB" % (name, label, v, (t + 1) * N * 32 >> 20))
                med = {}
                for P in (int(x) for x in a.pairs.split(",")):
                    lib.ctx_set_policy(ctx, "SUMCHECK_LANE_PAIRS", P)
                    T = {k: [] for k in ("begin", "round 1", "round 2 (fused)", "rounds 3 .. v + finish", "whole run, begin excluded",
                                         "unfused: mle_fix k = 1", "unfused: round 1 on the folded tables", "unfused round 2, sum")}
                    for rep in range(a.warmup + a.reps):
                        t0 = time.perf_counter()
                        sc = g.sumcheck_dev(label, vp(d_t), vp(d_w), v)
                        t1 = time.perf_counter()
                        sc.round(None)
                        t2 = time.perf_counter()
                        sc.round(ch[0])
                        t3 = time.perf_counter()
                        for j in range(2, v):
                            sc.round(ch[j - 1])
                        sc.finish(ch[-1])
                        t4 = time.perf_counter()
                        sc.close()
                        u0 = time.perf_counter()
                        lib.mle_fix_fr_dev(ctx, cid, vp(d_all), v, t + 1, pb(ch[:1]), 1, vp(d_fold))
                        u1 = time.perf_counter()
                        sc = g.sumcheck_dev(label, vp(d_fold), vp(d_fold) + t * (N // 2) * 32, v - 1)
                        u2 = time.perf_counter()
                        sc.round(None)
                        u3 = time.perf_counter()
                        sc.close()
                        if rep >= a.warmup:
                            for k, dt in (("begin", t1 - t0), ("round 1", t2 - t1), ("round 2 (fused)", t3 - t2), ("rounds 3 .. v + finish", t4 - t3),
                                          ("whole run, begin excluded", t4 - t1), ("unfused: mle_fix k = 1", u1 - u0),
                                          ("unfused: round 1 on the folded tables", u3 - u2), ("unfused round 2, sum", u1 - u0 + u3 - u2)):
                                T[k].append(dt * 1e3)
                    say(" SUMCHECK_LANE_PAIRS = %d" % P)
                    for k, ts in T.items():
                        med[(P, k)] = stat(k, ts)
                    say("  fused round 2 / unfused = %.3f" % (med[(P, "round 2 (fused)")] / med[(P, "unfused round 2, sum")]))
                lib.ctx_set_policy(ctx, "SUMCHECK_LANE_PAIRS", 0)
                ts_copy, ts_q = [], []
                for rep in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    d_copy.copy_(d_all)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    g.quotient_dev(label, vp(d_z), M, vp(d_h))
                    t2 = time.perf_counter()
                    if rep >= a.warmup:
                        ts_copy.append((t1 - t0) * 1e3)
                        ts_q.append((t2 - t1) * 1e3)
                say(" yardsticks")
                c = stat("(i) device-to-device copy of (t + 1) N Fr", ts_copy)
                stat("(ii) ark355_gr1cs_quotient_dev, same system", ts_q)
                best = min((int(x) for x in a.pairs.split(",")), key=lambda P: med[(P, "whole run, begin excluded")])
                say("  round 1 / copy = %.2f at the default; best whole run at SUMCHECK_LANE_PAIRS = %d"
                    % (med[(1, "round 1")] / c if (1, "round 1") in med else float("nan"), best))
                g.free()
                del d_t, d_all, d_fold, d_copy, d_h
            # the primitives alone on one table
            T = {k: [] for k in ("mle_eq_fr_dev", "mle_fix_fr_dev k = 1", "mle_eval_fr_dev", "(i) device-to-device copy of N Fr")}
            src = d_w
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                lib.mle_eq_fr_dev(ctx, cid, v, pb(tau), vp(d_one))
                t1 = time.perf_counter()
                lib.mle_fix_fr_dev(ctx, cid, vp(src), v, 1, pb(ch[:1]), 1, vp(d_half))
                t2 = time.perf_counter()
                lib.mle_eval_fr_dev(ctx, cid, vp(src), v, 1, pb(ch), vp(d_val))
                t3 = time.perf_counter()
                d_one.copy_(src)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                if rep >= a.warmup:
                    for k, dt in zip(T, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                        T[k].append(dt * 1e3)
            say("%s, primitives on one table, N = 2^%d (%d MiB)" % (name, v, N * 32 >> 20))
            for k, ts in T.items():
                stat(k, ts)
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
