#!/usr/bin/env python3
"""Quotient micro-benchmark: ark355_gr1cs_quotient_dev on three systems, both curves.
  (a) an R1CS-shaped predicate at N = 2^21: the 2^20-row mul-chain bench circuit plus its ell instance rows (A row n + i = e_i, B
      and C empty), z and h in device memory.  Next to it, on the same instance in the same process: ark355_witness_map (the
      six-transform route of the Groth16 prover, a HOST entry: z copied from page-locked memory, h copied back) and
      ark355_gr1cs_quotient (the host entry of the generic route, the same two copies) -- the like-for-like pair;
  (b) the SR1CS system of that R1CS (2 n + P rows, N = 2^22) through ark355_sr1cs_assignment_dev -> ark355_gr1cs_quotient_dev;
  (c) a degree-3 predicate of arity 4 at N = 2^18 (D = 2: transforms of 2^19 points).
The readings are interleaved after a warm-up of every call; each line gives the median, the minimum and the spread over the repeats.
Host-clock times of synchronous calls (each returns after a stream synchronise).  The box's multiply-add rate
(ark355_diag_mad_rate) is read before and after.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script of
its own.  Dev tool; run on an MI355X:  python tools/quotient_bench.py [--log-n 20] [--reps 20] [--out profiles/quotient_bench.txt]"""
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


def r1cs_predicate(cv, r1):
    """the instance's A, B, C with ell rows appended: A row n + i = e_i, B and C empty"""
    one = cv.fr_mont(1)
    ell, n = r1.ell, r1.n
    rp, col, cf = r1.row_ptr, r1.col, r1.coeff
    rps = [np.concatenate([rp[0], rp[0][-1] + np.arange(1, ell + 1, dtype=np.uint64)])]
    cols = [np.concatenate([col[0], np.arange(ell, dtype=np.uint32)])]
    cfs = [bytes(cf[0]) + one * ell]
    for k in (1, 2):
        rps.append(np.concatenate([rp[k], np.full(ell, rp[k][-1], dtype=np.uint64)]))
        cols.append(col[k])
        cfs.append(cf[k])
    terms = [(1, [(0, 1), (1, 1)]), (cv.r - 1, [(2, 1)])]
    return Predicate("R1CS", 3, terms, n + ell, rps, cols, cfs)


def degree3_predicate(cv, n, m):
    """5 x0 x1 x2 + x0^3 - 7 x2^2 - x3 over one-entry rows: entry (1, 1 + (i (k + 3)) mod (m - 1)) in matrix k"""
    i = np.arange(n, dtype=np.int64)
    rp = np.arange(n + 1, dtype=np.uint64)
    one = np.frombuffer(cv.fr_mont(1), dtype=np.uint8)
    cols = [(1 + (i * (k + 3)) % (m - 1)).astype(np.uint32) for k in range(4)]
    p = cv.r
    terms = [(5, [(0, 1), (1, 1), (2, 1)]), (1, [(0, 2), (0, 1)]), (p - 7, [(1, 0), (2, 2)]), (p - 1, [(3, 1)])]
    return Predicate("deg3", 4, terms, n, [rp] * 4, cols, [np.tile(one, n).tobytes()] * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--log-n3", type=int, default=18, help="log2 of the rows of the degree-3 predicate")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "quotient_bench measures on the GPU: there is nothing to report without one"
    n = 1 << a.log_n
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def dev(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    say("quotient_bench: mul-chain, n = 2^%d rows, %d interleaved repeats after %d warm-up rounds; ms per call (host clock around "
        "synchronous calls)" % (a.log_n, a.reps, a.warmup))
    say("box before: %.2f T v_mad_u64_u32/s (ark355_diag_mad_rate)" % lib.diag_mad_rate(ctx, 20.0)["tmad_per_s"])
    for name in a.curves.split(","):
        cv = params.CURVES[name]
        r1, z = synthetic.mulchain(cv, n)
        m = r1.ell + r1.w
        h_r1 = lib.r1cs_load(ctx, cv.curve_id, n, r1.ell, r1.w, list(zip(r1.row_ptr, r1.col, r1.coeff)))
        z_host = torch.from_numpy(np.frombuffer(synthetic.z_to_mont_bytes(cv, z), dtype=np.uint8).copy()).pin_memory()
        d_z = z_host.cuda()
        # (a)
        ga = GR1CS(cv, r1.ell, r1.w, [r1cs_predicate(cv, r1)]).load(lib, ctx)
        da = ga.quotient_dims("R1CS")
        assert da[3] == lib.dll.ark355_r1cs_domain_size(h_r1) == 2 * n
        d_ha = dev(da[3] * 32)
        h_host = torch.zeros(da[3] * 32, dtype=torch.uint8).pin_memory()
        # (b)
        s = lib.sr1cs_from_r1cs(ctx, h_r1)
        ell2, w2, rows, _ = lib.sr1cs_dims(s)
        sysb = lib.sr1cs_system(s)
        db = lib.gr1cs_quotient_dims(sysb, 0)
        d_zp, d_hb = dev((ell2 + w2) * 32), dev(db[3] * 32)
        # (c)
        n3, m3 = 1 << a.log_n3, 64
        gc3 = GR1CS(cv, 1, m3 - 1, [degree3_predicate(cv, n3, m3)]).load(lib, ctx)
        dc = gc3.quotient_dims("deg3")
        rnd = np.random.default_rng(0x355)
        z3 = [1] + [int.from_bytes(rnd.bytes(31), "little") for _ in range(m3 - 1)]
        d_z3 = torch.from_numpy(np.frombuffer(synthetic.z_to_mont_bytes(cv, z3), dtype=np.uint8).copy()).cuda()
        d_hc = dev(dc[3] * 32)
        torch.cuda.synchronize()
        vp = lambda t: t.data_ptr()                            # noqa: E731
        import ctypes as C

        def call_a():
            ga.quotient_dev("R1CS", vp(d_z), m, vp(d_ha))

        def call_a_host():
            lib.check(ctx, lib.dll.ark355_gr1cs_quotient(ctx, ga.handle, 0, C.c_void_p(vp(z_host)), m, 0, C.c_void_p(vp(h_host))))

        def call_wm():
            lib.check(ctx, lib.dll.ark355_witness_map(ctx, h_r1, C.c_void_p(vp(z_host)), m, C.c_void_p(vp(h_host))))

        def call_b():
            lib.sr1cs_assignment_dev(ctx, s, vp(d_z), m, vp(d_zp))
            lib.gr1cs_quotient_dev(ctx, sysb, 0, vp(d_zp), ell2 + w2, 0, vp(d_hb))

        def call_c():
            gc3.quotient_dev("deg3", vp(d_z3), m3, vp(d_hc))

        calls = [("(a) ark355_gr1cs_quotient_dev, R1CS shape", call_a), ("(a') ark355_gr1cs_quotient, pinned z and h", call_a_host),
                 ("(a'') ark355_witness_map, pinned z and h", call_wm), ("(b) sr1cs_assignment_dev -> gr1cs_quotient_dev", call_b),
                 ("(c) ark355_gr1cs_quotient_dev, degree 3", call_c)]
        # the two routes compute the same bytes
        call_wm()
        want = h_host.numpy().tobytes()
        call_a_host()
        assert h_host.numpy().tobytes() == want
        call_a()
        assert d_ha.cpu().numpy().tobytes() == want
        for _ in range(a.warmup):
            for _, f in calls:
                f()
        t = [[] for _ in calls]
        for _ in range(a.reps):
            for k, (_, f) in enumerate(calls):
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        say("%s: (a) %d rows, N = 2^%d; (b) %d rows, N = 2^%d; (c) %d rows, degree %d, N = 2^%d, D = %d"
            % (name, n + r1.ell, da[1], rows, db[1], n3, dc[0], dc[1], 1 << dc[2]))
        med = []
        for (label, _), ts in zip(calls, t):
            q = statistics.quantiles(ts, n=4)
            med.append(statistics.median(ts))
            say("  %-52s median %8.3f  min %8.3f  max-min %7.3f  iqr %6.3f" % (label, med[-1], min(ts), max(ts) - min(ts), q[2] - q[0]))
        say("  (a') / (a'') = %.3f, host entries with the same two copies; seven transforms against six give 7/6 = 1.167"
            % (med[1] / med[2]))
        gc3.free()
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
