#!/usr/bin/env python3
"""Generator A/B: the Groth16 key of the bench circuit (snark_amd.synthetic.mulchain, 2^log_n constraints) made resident by

  host      the route before ark355_setup: ark355_setup_scalars on host threads, two ark355_fixed_base_mul calls for the
            six single points and six for the vectors (gamma_abc, a, b_g1, b_g2, h, l), then ark355_pk_load of the host
            vectors;
  device    ark355_setup returning only the resident handle (out = NULL);
  device+b  ark355_setup returning the handle AND every vector of the key in host memory.

Every run is its own child process under `timeout -k 10` (fresh context, cold tables, nothing shared between runs); the
three routes alternate --reps times and the medians are printed.  The clock is the host's, around the calls of the route
alone: building the statement and ark355_r1cs_load (both routes need the matrices resident for proving anyway) are listed
beside it.  All routes go through ctypes into preallocated numpy buffers, so no route pays for a Python-side copy.
A child that fails ends the job: nothing more is started on the device.

  python tools/setup_bench.py [--log-n 20] [--curves bls12_381,bn254] [--reps 3] [--out profiles/setup_bench.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/setup_bench.py --child device --curve bls12_381
                                      (one setup in this process, for the per-kernel table)"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

ROUTES = ("host", "device", "device+b")


def child(route, curve_name, log_n):
    import numpy as np
    import snark_amd
    from snark_amd import params, synthetic
    from snark_amd._binding import SETUP_OUT_FIELDS, PkDesc, SetupOut
    cv = params.CURVES[curve_name]
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    sz = lib.sizes(cv.curve_id)
    g1s, g2s = sz["g1"], sz["g2"]
    t0 = time.perf_counter()
    r1, _ = synthetic.mulchain(cv, 1 << log_n)
    t_build = time.perf_counter() - t0
    rnd = random.Random(0x355)
    td = b"".join(cv.fr_canon(rnd.randrange(1, cv.r)) for _ in range(5))
    mats = list(zip(r1.row_ptr, r1.col, r1.coeff))
    ell, w, m, N = r1.ell, r1.w, r1.m, r1.domain_size
    t0 = time.perf_counter()
    rh = lib.r1cs_load(ctx, cv.curve_id, r1.n, ell, w, mats)
    t_r1cs = time.perf_counter() - t0
    g1, g2 = cv.g1_gen_raw(), cv.g2_gen_raw()
    nbytes = dict(alpha_g1=g1s, beta_g1=g1s, delta_g1=g1s, beta_g2=g2s, gamma_g2=g2s, delta_g2=g2s, gamma_abc_g1=ell * g1s,
                  a_query=m * g1s, b_g1_query=m * g1s, b_g2_query=m * g2s, h_query=(N - 1) * g1s, l_query=w * g1s)
    bufs = {k: np.zeros(max(1, v), dtype=np.uint8) for k, v in nbytes.items()}
    h = C.c_void_p()
    stages = {}
    t0 = time.perf_counter()
    if route == "host":
        sc = lib.setup_scalars(cv.curve_id, r1.n, ell, w, mats, td)
        stages["setup_scalars"] = time.perf_counter() - t0

        def mul(group, scalars, out):
            s = np.ascontiguousarray(scalars)
            base = np.frombuffer(g1 if group == 1 else g2, dtype=np.uint8)
            lib.check(ctx, lib.dll.ark355_fixed_base_mul(ctx, cv.curve_id, group, base.ctypes.data_as(C.c_void_p),
                                                         s.ctypes.data_as(C.c_void_p), len(s) // 32,
                                                         out.ctypes.data_as(C.c_void_p)))
        t1 = time.perf_counter()
        tdv = np.frombuffer(td, dtype=np.uint8)
        one1, one2 = np.zeros(3 * g1s, dtype=np.uint8), np.zeros(3 * g2s, dtype=np.uint8)
        mul(1, np.concatenate([tdv[32:64], tdv[64:96], tdv[128:160]]), one1)
        mul(2, np.concatenate([tdv[64:96], tdv[96:128], tdv[128:160]]), one2)
        mul(1, sc["gamma_abc"], bufs["gamma_abc_g1"])
        mul(1, sc["u"], bufs["a_query"])
        mul(1, sc["v"], bufs["b_g1_query"])
        mul(2, sc["v"], bufs["b_g2_query"])
        mul(1, sc["h"], bufs["h_query"])
        mul(1, sc["l"], bufs["l_query"])
        stages["fixed_base_mul_x8"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        d = PkDesc()
        d.num_instance, d.num_witness, d.domain_size = ell, w, N
        for k in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query"):
            setattr(d, k, bufs[k].ctypes.data)
        d.alpha_g1, d.beta_g1, d.delta_g1 = one1.ctypes.data, one1.ctypes.data + g1s, one1.ctypes.data + 2 * g1s
        d.beta_g2, d.delta_g2 = one2.ctypes.data, one2.ctypes.data + 2 * g2s
        lib.check(ctx, lib.dll.ark355_pk_load(ctx, cv.curve_id, C.byref(d), C.byref(h)))
        stages["pk_load"] = time.perf_counter() - t1
    else:
        so = None
        if route == "device+b":
            so = SetupOut()
            for k in SETUP_OUT_FIELDS:
                if k in bufs:
                    setattr(so, k, bufs[k].ctypes.data)
        b1, b2, tb = (np.frombuffer(x, dtype=np.uint8) for x in (g1, g2, td))
        lib.check(ctx, lib.dll.ark355_setup(ctx, rh, b1.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p),
                                            tb.ctypes.data_as(C.c_void_p), C.byref(so) if so is not None else None, C.byref(h)))
    total = time.perf_counter() - t0
    assert lib.pk_dims(h) == (ell, w, N)
    lib.dll.ark355_pk_free(h)
    lib.dll.ark355_r1cs_free(rh)
    lib.ctx_destroy(ctx)
    print(json.dumps({"route": route, "curve": curve_name, "log_n": log_n, "seconds": round(total, 4),
                      "stages": {k: round(v, 4) for k, v in stages.items()}, "statement_s": round(t_build, 3),
                      "r1cs_load_s": round(t_r1cs, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--curve", default="bls12_381", help="with --child")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=ROUTES)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.curve, a.log_n)
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for curve in a.curves.split(","):
        secs = {r: [] for r in ROUTES}
        for rep in range(a.reps):
            for route in ROUTES:
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", route,
                       "--curve", curve, "--log-n", str(a.log_n)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:        # a fault, an abort or the time limit: nothing more is started on the device
                    print("child %s %s ended with status %d\n%s" % (route, curve, r.returncode, r.stderr[-2000:]), flush=True)
                    return r.returncode
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                secs[route].append(rec["seconds"])
                say("run %d %s" % (rep, json.dumps(rec)))
        med = {r: statistics.median(v) for r, v in secs.items()}
        say("median %s 2^%d: host route %.3f s | device, handle only %.3f s (%.2fx) | device, handle + key bytes %.3f s (%.2fx)"
            % (curve, a.log_n, med["host"], med["device"], med["host"] / med["device"], med["device+b"],
               med["host"] / med["device+b"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("setup_bench: generator routes, one child process per run, alternated; seconds on the host clock\n\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
