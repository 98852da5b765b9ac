#!/usr/bin/env python3
"""Micro-benchmark of the openings in the evaluation basis: ark355_evals_eval_fr_dev and ark355_evals_div_linear_fr_dev (out of
place and in place) at 2^21 and 2^22 points with count 1 and 4, both curves, x outside the domain, against three yardsticks from the
same run, none of them the code under test:
  (i)   a device-to-device copy of the same bytes: the traffic floor;
  (ii)  the route a caller had before these entries.  Evaluation: ark355_ntt_fr_dev (inverse) per vector, then
        ark355_poly_eval_fr_dev.  Division: the inverse transform per vector, ark355_poly_div_linear_fr_dev, the forward transform
        per vector.  The transforms run in place, so the data of route (ii) changes from repeat to repeat: any words below r are an
        input;
  (iii) ark355_lagrange_fr_dev of the same log_n: the kernel that pays one field inversion per 8 points, where the entries under
        test pay one per workgroup (2048 points at the default EVALS_LANE_POINTS).
The readings are interleaved after a warm-up of every call; each line gives the median, the minimum and the spread over the
repeats.  Host-clock times of synchronous calls (each returns after a stream synchronise).  The box's multiply-add rate
(ark355_diag_mad_rate) is read before and after.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script
of its own (--yardsticks 0).  Dev tool; run on an MI355X:
  python tools/evals_bench.py [--logs 21,22] [--reps 20] [--out profiles/evals_bench.txt]"""
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

X = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="21,22")
    ap.add_argument("--counts", default="1,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--yardsticks", type=int, default=1, help="0: only the entries under test (a traced run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "evals_bench measures on the GPU: there is nothing to report without one"
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("evals_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock around synchronous calls); "
        "EVALS_LANE_POINTS = %d" % (a.reps, a.warmup, lib.ctx_get_policy(ctx, "EVALS_LANE_POINTS")))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    xb = X.to_bytes(32, "little")
    rng = np.random.default_rng(0xE5)
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        top = (1 << ((cv.r >> 248).bit_length() - 1)) - 1      # words below r: valid Montgomery images
        for log_n in (int(v) for v in a.logs.split(",")):
            n = 1 << log_n
            for count in (int(v) for v in a.counts.split(",")):
                words = rng.integers(0, 256, size=(count * n, 32), dtype=np.uint8)
                words[:, 31] &= top
                d_e = torch.from_numpy(words.reshape(-1)).cuda()
                d_q = torch.zeros(count * n * 32, dtype=torch.uint8, device="cuda")
                d_w = d_e.clone()                              # divided in place, over and over
                d_c = d_e.clone()                              # route (ii) transforms it in place
                d_o = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
                d_l = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                d_s = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                vp = lambda t: t.data_ptr()                    # noqa: E731

                def call_eval():
                    lib.evals_eval_fr_dev(ctx, cv.curve_id, vp(d_e), log_n, count, 0, xb, vp(d_o))

                def call_div():
                    lib.evals_div_linear_fr_dev(ctx, cv.curve_id, vp(d_e), log_n, count, 0, xb, vp(d_q), vp(d_o))

                def call_div_in_place():
                    lib.evals_div_linear_fr_dev(ctx, cv.curve_id, vp(d_w), log_n, count, 0, xb, vp(d_w), vp(d_o))

                def call_copy():
                    d_q.copy_(d_e)
                    torch.cuda.synchronize()

                def call_route_eval():
                    for k in range(count):                     # queued on the context's stream; poly_eval waits for all of it
                        lib.ntt_dev(ctx, cv.curve_id, vp(d_c) + k * n * 32, vp(d_s), log_n, inverse=True)
                    lib.poly_eval_fr_dev(ctx, cv.curve_id, vp(d_c), n, count, xb, vp(d_o))

                def call_route_div():
                    for k in range(count):
                        lib.ntt_dev(ctx, cv.curve_id, vp(d_c) + k * n * 32, vp(d_s), log_n, inverse=True)
                    lib.poly_div_linear_fr_dev(ctx, cv.curve_id, vp(d_c), n, count, xb, vp(d_c), vp(d_o))
                    for k in range(count):
                        lib.ntt_dev(ctx, cv.curve_id, vp(d_c) + k * n * 32, vp(d_s), log_n, inverse=False)
                    torch.cuda.synchronize()

                def call_lagrange():
                    lib.lagrange_fr_dev(ctx, cv.curve_id, log_n, xb, vp(d_l))

                calls = [("evals_eval_dev", call_eval), ("evals_div_linear_dev", call_div),
                         ("evals_div_linear_dev in place", call_div_in_place)]
                if a.yardsticks:
                    calls += [("(i) device-to-device copy", call_copy), ("(ii) ntt^-1 + poly_eval", call_route_eval),
                              ("(ii) ntt^-1 + poly_div_linear + ntt", call_route_div),
                              ("(iii) ark355_lagrange_fr_dev, one vector", call_lagrange)]
                for _ in range(a.warmup):
                    for _, f in calls:
                        f()
                t = [[] for _ in calls]
                for _ in range(a.reps):
                    for k, (_, f) in enumerate(calls):
                        t0 = time.perf_counter()
                        f()
                        t[k].append((time.perf_counter() - t0) * 1e3)
                say("%s: N = 2^%d, count = %d (%d MiB)" % (name, log_n, count, count * n * 32 >> 20))
                med = {}
                for (label, _), ts in zip(calls, t):
                    q = statistics.quantiles(ts, n=4)
                    med[label] = statistics.median(ts)
                    say("  %-42s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, med[label], min(ts), max(ts) - min(ts), q[2] - q[0]))
                if a.yardsticks:
                    c = med["(i) device-to-device copy"]
                    say("  eval / copy = %.2f   div / copy = %.2f   eval / route (ii) = %.3f   div / route (ii) = %.3f   "
                        "eval per vector / lagrange = %.3f"
                        % (med["evals_eval_dev"] / c, med["evals_div_linear_dev"] / c, med["evals_eval_dev"] / med["(ii) ntt^-1 + poly_eval"],
                           med["evals_div_linear_dev"] / med["(ii) ntt^-1 + poly_div_linear + ntt"],
                           med["evals_eval_dev"] / count / med["(iii) ark355_lagrange_fr_dev, one vector"]))
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
