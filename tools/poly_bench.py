#!/usr/bin/env python3
"""Polynomial-opening micro-benchmark: ark355_poly_eval_fr_dev, ark355_poly_div_linear_fr_dev (out of place and in place) and
ark355_poly_lincomb_fr_dev (count = 4) at len = 2^21 and 2^22 -- the h of the bench circuit's R1CS and SR1CS shapes -- with
count 1 and 4, both curves, against three yardsticks from the same run, none of them the code under test:
  (i)   a device-to-device copy of the same bytes: the traffic floor (eval reads 32 len bytes, div reads and writes them);
  (ii)  one ark355_ntt_fr_dev of the same length: an existing entry over the same data;
  (iii) the route a caller had before these entries: the polynomial to pageable host memory and back, two copies and no host
        arithmetic.
The readings are interleaved after a warm-up of every call; each line gives the median, the minimum and the spread over the
repeats.  Host-clock times of synchronous calls (each returns after a stream synchronise).  The box's multiply-add rate
(ark355_diag_mad_rate) is read before and after.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script
of its own.  Dev tool; run on an MI355X:
  python tools/poly_bench.py [--logs 21,22] [--reps 20] [--out profiles/poly_bench.txt]"""
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
    assert torch.cuda.is_available(), "poly_bench measures on the GPU: there is nothing to report without one"
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("poly_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock around synchronous calls); "
        "POLY_LANE_COEFFS = %d" % (a.reps, a.warmup, lib.ctx_get_policy(ctx, "POLY_LANE_COEFFS")))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    xb = X.to_bytes(32, "little")
    rng = np.random.default_rng(0xB5)
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        top = (1 << ((cv.r >> 248).bit_length() - 1)) - 1      # words below r: valid Montgomery images
        for log_n in (int(v) for v in a.logs.split(",")):
            n = 1 << log_n
            for count in (int(v) for v in a.counts.split(",")):
                words = rng.integers(0, 256, size=(count * n, 32), dtype=np.uint8)
                words[:, 31] &= top
                d_p = torch.from_numpy(words.reshape(-1)).cuda()
                d_q = torch.zeros(count * n * 32, dtype=torch.uint8, device="cuda")
                d_w = d_p.clone()                              # divided in place, over and over: any words below r are an input
                d_o = torch.zeros(count * 32, dtype=torch.uint8, device="cuda")
                d_l = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                d_n = d_p[:n * 32].clone()
                d_s = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                host = np.empty(count * n * 32, dtype=np.uint8)                # pageable
                scal = b"".join(int(v).to_bytes(32, "little") for v in (1, X, X * X % cv.r, X * X * X % cv.r))
                torch.cuda.synchronize()
                vp = lambda t: t.data_ptr()                    # noqa: E731

                def call_eval():
                    lib.poly_eval_fr_dev(ctx, cv.curve_id, vp(d_p), n, count, xb, vp(d_o))

                def call_div():
                    lib.poly_div_linear_fr_dev(ctx, cv.curve_id, vp(d_p), n, count, xb, vp(d_q), vp(d_o))

                def call_div_in_place():
                    lib.poly_div_linear_fr_dev(ctx, cv.curve_id, vp(d_w), n, count, xb, vp(d_w), vp(d_o))

                def call_lincomb():
                    lib.poly_lincomb_fr_dev(ctx, cv.curve_id, vp(d_p), n, 4, scal, vp(d_l))

                def call_copy():
                    d_q.copy_(d_p)
                    torch.cuda.synchronize()

                def call_ntt():
                    lib.ntt_dev(ctx, cv.curve_id, vp(d_n), vp(d_s), log_n)     # queued on the context's stream, not waited for
                    torch.cuda.synchronize()

                def call_host_route():
                    host_t = torch.from_numpy(host)
                    host_t.copy_(d_p)
                    d_q.copy_(host_t)
                    torch.cuda.synchronize()

                calls = [("eval_dev", call_eval), ("div_linear_dev", call_div), ("div_linear_dev in place", call_div_in_place)]
                if count == 4:
                    calls.append(("lincomb_dev, count = 4", call_lincomb))
                if a.yardsticks:
                    calls += [("(i) device-to-device copy", call_copy), ("(ii) ark355_ntt_fr_dev, one polynomial", call_ntt),
                              ("(iii) to pageable host memory and back", call_host_route)]
                for _ in range(a.warmup):
                    for _, f in calls:
                        f()
                t = [[] for _ in calls]
                for _ in range(a.reps):
                    for k, (_, f) in enumerate(calls):
                        t0 = time.perf_counter()
                        f()
                        t[k].append((time.perf_counter() - t0) * 1e3)
                say("%s: len = 2^%d, count = %d (%d MiB)" % (name, log_n, count, count * n * 32 >> 20))
                med = {}
                for (label, _), ts in zip(calls, t):
                    q = statistics.quantiles(ts, n=4)
                    med[label] = statistics.median(ts)
                    say("  %-42s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, med[label], min(ts), max(ts) - min(ts), q[2] - q[0]))
                if a.yardsticks:
                    c = med["(i) device-to-device copy"]
                    say("  eval / copy = %.2f   div / copy = %.2f   div in place / copy = %.2f   div / host route = %.3f"
                        % (med["eval_dev"] / c, med["div_linear_dev"] / c, med["div_linear_dev in place"] / c,
                           med["div_linear_dev"] / med["(iii) to pageable host memory and back"]))
    say("box after: %.2f T v_mad_u64_u32/s" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lib.ctx_destroy(ctx)


if __name__ == "__main__":
    main()
