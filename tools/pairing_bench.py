#!/usr/bin/env python3
"""Pairing micro-benchmark: `ark355_multi_pairing` and `ark355_verify_batch`, host route (PAIRING_DEVICE=0: Miller loops,
curve checks and rho_j A_j on at most 16 host threads) against device route (PAIRING_DEVICE=1: the kernels of
snark_amd/csrc/pairing_impl.cuh), both curves, 1 .. 16384 pairs.

The four readings of a size (multi_pairing host / device, verify_batch host / device) are interleaved in one process, after
one warm-up of each; every figure is the median of --reps runs of a synchronous call on the host clock, inputs in pageable
host memory (uploads included, as a caller sees them).  `verify_batch` of n proofs runs n + 3 Miller loops.  The library
reports its phases on stderr under policy TRACE_HOST (curve checks, scalar multiplications, Miller loops, final
exponentiation); the child reads them back, so the final exponentiation -- host code on both routes, once per call -- and
the rho_j A_j step are listed on their own.  The pairs are a_i G1, b_i G2 with random a_i, b_i; the proofs are eight
oracle-made proofs of one key, cycled, each with its own 128-bit rho.

The last lines give, per curve and entry, the smallest size from which the device route is at least 10 % faster at that size
and at every larger one: policy.h's PAIRING_DEVICE_MIN is that figure for the slower curve.

--each measures the per-group entries by the same protocol: `ark355_pairing_groups(n, 1)` and `ark355_verify_each(n)`, host
route (one final exponentiation per group on at most 16 host threads; run up to --host-max groups only, beyond that it is
seconds per call) against device route (final exponentiations in pairing_final_exp_kernel), with the `ark355_verify_batch`
device time of the same n proofs beside it: what a per-proof answer costs over a yes/no.  policy.h's PAIRING_EACH_MIN is the
crossover of the slower curve and the slower entry.

--pvk measures the processed verifying key by the same protocol: `ark355_verify_each` (the yardstick: this entry redoes the
per-key work on every call) beside `ark355_verify_each_pvk` on a handle made once, and `ark355_vk_process` itself (process +
free), at 1 proof on the host route and 256 .. 16384 proofs on the device route.  Besides the medians it prints the spread
(min .. max) of the yardstick's readings: the processed entry does strictly less work, so it must not be slower than the
yardstick by more than that spread.

--from-bytes measures proofs arriving as ark-serialize bytes (compressed, VALIDATE_FULL; 4096 and 65536 proofs): the path
without the bytes entries -- a host loop of `ark355_proof_from_bytes`, then `ark355_verify_each_pvk`, run up to --host-max
proofs -- beside `ark355_verify_each_bytes`, and the decode stage alone (`ark355_proofs_from_bytes`).  --lib PATH runs the
same legs on another build of the library: one built with -DARK_WIRE_SUBGROUP_RP (tools/build_variant.sh) keeps the `[r]P`
subgroup test in its decoders, so its host loop is the loop as it was before the endomorphism tests and its decode stage
states their gain apart from the gain of decoding on the device.

One child process per curve, each under its own `timeout`.  Dev tool; run on an MI355X:
  python tools/pairing_bench.py [--reps 5] [--out profiles/pairing_bench.txt]
  python tools/pairing_bench.py --each [--reps 5] [--out profiles/pairing_each_bench.txt]
  python tools/pairing_bench.py --pvk [--reps 5] [--out profiles/pvk_bench.txt]
  python tools/pairing_bench.py --from-bytes [--lib variants/lib_rp.so] [--out profiles/verify_bytes_bench.txt]
  rocprofv3 --kernel-trace --output-format csv -- python tools/pairing_bench.py --from-bytes --child bls12_381 --host-max 0
                                      (proof_decode_kernel alone: the stage's figure includes the copies; add --lib for the [r]P build)
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pairing_bench.py --one-verify-each 4096
                                      (one BLS12-381 verify_each, for profiles/pairing_each_kernel_stats.csv)
  rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pairing_bench.py --one-verify 4096
                                      (one BLS12-381 verify_batch under the default policy, for profiles/pairing_kernel_stats.csv)"""
import argparse
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [1, 4, 16, 64, 256, 1024, 4096, 16384]
EACH_SIZES = [1, 4, 16, 32, 64, 128, 256, 512, 1024, 4096]
PVK_SIZES = [1, 256, 1024, 4096, 16384]          # 1: the host route (verify_with_processed_vk of one proof); the others: device
PHASE = re.compile(r"\[ark355\] (\w+) route=(\w+) pairs=(\d+) check_ms=([\d.]+) scalar_mul_ms=([\d.]+)"
                   r"(?: miller_ms=([\d.]+) final_exp_ms=([\d.]+))?")


def child(curve_name, reps, sizes):
    import snark_amd
    import pairing_cases as P
    from oracle import serialize as Z
    from oracle.fields import BLS12_381, BN254
    C = {"bls12_381": BLS12_381, "bn254": BN254}[curve_name]
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lib.ctx_set_policy(ctx, "TRACE_HOST", 1)
    sz = lib.sizes(C.curve_id)
    rnd = random.Random(71)
    nmax = max(sizes)
    a = [rnd.randrange(1, C.r) for _ in range(nmax)]
    b = [rnd.randrange(1, C.r) for _ in range(nmax)]
    g1, g2 = P.points_with_dlogs(lib, ctx, C, a, b, cross_check=1)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(nmax)]

    # the library's phase lines arrive on fd 2: point it at a file for the length of the measurement
    trace = tempfile.TemporaryFile(mode="w+")
    saved = os.dup(2)
    os.dup2(trace.fileno(), 2)
    rows = []
    try:
        for n in sizes:
            p1, p2 = g1[:n * sz["g1"]], g2[:n * sz["g2"]]
            ps = [proofs[j % 8] for j in range(n)]
            xs = b"".join(inputs[j % 8] for j in range(n))
            rh = rho[:n] if n > 1 else None

            def mp(route):
                lib.ctx_set_policy(ctx, "PAIRING_DEVICE", route)
                return lib.multi_pairing(ctx, C.curve_id, p1, p2, n)

            def vb(route):
                lib.ctx_set_policy(ctx, "PAIRING_DEVICE", route)
                assert lib.verify_batch(ctx, C.curve_id, vk, ps, xs, rh)

            calls = [("mp_host", lambda: mp(0)), ("mp_dev", lambda: mp(1)), ("vb_host", lambda: vb(0)), ("vb_dev", lambda: vb(1))]
            assert mp(0) == mp(1)                      # warm-up of both routes, and they agree byte for byte
            vb(0)
            vb(1)
            t = {k: [] for k, _ in calls}
            ph = {k: [] for k, _ in calls}
            for _ in range(reps):
                for k, f in calls:
                    trace.seek(0, os.SEEK_END)
                    pos = trace.tell()
                    t0 = time.perf_counter()
                    f()
                    t[k].append((time.perf_counter() - t0) * 1e3)
                    trace.seek(pos)
                    m = [PHASE.search(l) for l in trace.read().splitlines()]
                    m = [x for x in m if x]
                    if m:
                        ph[k].append([float(v) if v else float("nan") for v in m[-1].groups()[3:]])
            med = {k: statistics.median(v) for k, v in t.items()}

            def phase(k, i):
                v = [x[i] for x in ph[k] if x[i] == x[i]]
                return statistics.median(v) if v else float("nan")

            rows.append((n, med, {k: [phase(k, i) for i in range(4)] for k in t}))
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    lib.ctx_destroy(ctx)
    print("curve %s: ms per call, median of %d interleaved runs (host clock); speed-up = host / device" % (C.name, reps))
    print("%7s | %11s %11s %8s | %11s %11s %8s | %9s | %13s %13s | %11s %11s"
          % ("pairs", "mp host", "mp device", "speed-up", "vb host", "vb device", "speed-up", "final exp",
             "rho*A host", "rho*A device", "miller host", "miller dev"))
    for n, med, ph in rows:
        print("%7d | %11.3f %11.3f %8.2f | %11.3f %11.3f %8.2f | %9.3f | %13.3f %13.3f | %11.3f %11.3f"
              % (n, med["mp_host"], med["mp_dev"], med["mp_host"] / med["mp_dev"], med["vb_host"], med["vb_dev"],
                 med["vb_host"] / med["vb_dev"], ph["mp_dev"][3], ph["vb_host"][1], ph["vb_dev"][1], ph["mp_host"][2], ph["mp_dev"][2]))
    for entry, h, d in (("multi_pairing", "mp_host", "mp_dev"), ("verify_batch", "vb_host", "vb_dev")):
        cross = None
        for i in range(len(rows) - 1, -1, -1):
            if rows[i][1][d] * 1.10 <= rows[i][1][h]:
                cross = rows[i][0]
            else:
                break
        print("crossover %s %s: device route at least 10 %% faster from %s pairs on" % (C.name, entry, cross))
    print("", flush=True)


def child_each(curve_name, reps, sizes, host_max):
    import snark_amd
    import pairing_cases as P
    from oracle import serialize as Z
    from oracle.fields import BLS12_381, BN254
    C = {"bls12_381": BLS12_381, "bn254": BN254}[curve_name]
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    sz = lib.sizes(C.curve_id)
    rnd = random.Random(71)
    nmax = max(sizes)
    a = [rnd.randrange(1, C.r) for _ in range(nmax)]
    b = [rnd.randrange(1, C.r) for _ in range(nmax)]
    g1, g2 = P.points_with_dlogs(lib, ctx, C, a, b, cross_check=1)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(nmax)]
    rows = []
    for n in sizes:
        p1, p2 = g1[:n * sz["g1"]], g2[:n * sz["g2"]]
        ps = [proofs[j % 8] for j in range(n)]
        xs = b"".join(inputs[j % 8] for j in range(n))
        rh = rho[:n] if n > 1 else None

        def pg(route):
            lib.ctx_set_policy(ctx, "PAIRING_DEVICE", route)
            return lib.pairing_groups(ctx, C.curve_id, p1, p2, n, 1)

        def ve(route):
            lib.ctx_set_policy(ctx, "PAIRING_DEVICE", route)
            assert all(lib.verify_each(ctx, C.curve_id, vk, ps, xs))

        def vb():
            lib.ctx_set_policy(ctx, "PAIRING_DEVICE", 1)
            assert lib.verify_batch(ctx, C.curve_id, vk, ps, xs, rh)

        calls = [("pg_dev", lambda: pg(1)), ("ve_dev", lambda: ve(1)), ("vb_dev", vb)]
        if n <= host_max:
            calls += [("pg_host", lambda: pg(0)), ("ve_host", lambda: ve(0))]
            assert pg(0) == pg(1)                      # warm-up of both routes, and they agree byte for byte
            ve(0)
        else:
            pg(1)
        ve(1)
        vb()
        t = {k: [] for k, _ in calls}
        for _ in range(reps):
            for k, f in calls:
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        rows.append((n, {k: statistics.median(v) for k, v in t.items()}))
    lib.ctx_destroy(ctx)
    print("curve %s: ms per call, median of %d interleaved runs (host clock); speed-up = host / device" % (C.name, reps))
    print("%7s | %11s %11s %8s | %11s %11s %8s | %11s %9s"
          % ("n", "pg host", "pg device", "speed-up", "ve host", "ve device", "speed-up", "vb device", "ve / vb"))
    nan = float("nan")
    for n, med in rows:
        ph, vh = med.get("pg_host", nan), med.get("ve_host", nan)
        print("%7d | %11.3f %11.3f %8.2f | %11.3f %11.3f %8.2f | %11.3f %9.2f"
              % (n, ph, med["pg_dev"], ph / med["pg_dev"], vh, med["ve_dev"], vh / med["ve_dev"], med["vb_dev"],
                 med["ve_dev"] / med["vb_dev"]))
    measured = [r for r in rows if "pg_host" in r[1]]
    for entry, h, d in (("pairing_groups", "pg_host", "pg_dev"), ("verify_each", "ve_host", "ve_dev")):
        cross = None
        for n, med in reversed(measured):
            if med[d] * 1.10 <= med[h]:
                cross = n
            else:
                break
        print("crossover %s %s: device route at least 10 %% faster from %s groups / proofs on" % (C.name, entry, cross))
    print("", flush=True)


def child_pvk(curve_name, reps, sizes):
    import snark_amd
    import pairing_cases as P
    from oracle.fields import BLS12_381, BN254
    C = {"bls12_381": BLS12_381, "bn254": BN254}[curve_name]
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    pvk = lib.vk_process(ctx, C.curve_id, vk)
    info = lib.pvk_info(pvk)
    rows = []
    for n in sizes:
        route = 0 if n == 1 else 1
        lib.ctx_set_policy(ctx, "PAIRING_DEVICE", route)
        ps = [proofs[j % 8] for j in range(n)]
        xs = b"".join(inputs[j % 8] for j in range(n))

        def ve():
            return lib.verify_each(ctx, C.curve_id, vk, ps, xs)

        def vp():
            return lib.verify_each_pvk(ctx, pvk, ps, xs)

        def pr():
            lib.pvk_free(lib.vk_process(ctx, C.curve_id, vk))

        calls = [("ve", ve), ("ve_pvk", vp), ("process", pr)]
        assert ve() == vp() == [True] * n              # warm-up of both entries, and they agree
        pr()
        t = {k: [] for k, _ in calls}
        for _ in range(reps):
            for k, f in calls:
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        rows.append((n, route, t))
    lib.pvk_free(pvk)
    lib.ctx_destroy(ctx)
    print("curve %s: ms per call, median of %d interleaved runs (host clock); the handle holds %d bytes of HBM (num_instance %d)"
          % (C.name, reps, info["resident_bytes"], info["num_instance"]))
    print("%7s %6s | %11s %19s | %15s %8s %9s | %11s | %s"
          % ("proofs", "route", "verify_each", "(min .. max)", "verify_each_pvk", "saved", "speed-up", "vk_process", "verdict"))
    for n, route, t in rows:
        ve, vp = statistics.median(t["ve"]), statistics.median(t["ve_pvk"])
        spread = max(t["ve"]) - min(t["ve"])
        verdict = "ok" if vp <= ve + spread else "SLOWER than the yardstick by more than its spread"
        print("%7d %6s | %11.3f %19s | %15.3f %8.3f %9.2f | %11.3f | %s"
              % (n, "device" if route else "host", ve, "(%.3f .. %.3f)" % (min(t["ve"]), max(t["ve"])), vp, ve - vp, ve / vp,
                 statistics.median(t["process"]), verdict))
    print("", flush=True)


def child_bytes(curve_name, reps, sizes, host_max, lib_path):
    """Proofs from wire bytes (compressed, VALIDATE_FULL): the path without the bytes entries -- a host loop of
    ark355_proof_from_bytes, then ark355_verify_each_pvk -- beside ark355_verify_each_bytes, and the decode stage alone
    (ark355_proofs_from_bytes: upload, decode kernel, download).  --lib names another build of the library, e.g. one made with
    -DARK_WIRE_SUBGROUP_RP, whose decoders keep the [r]P subgroup test: its loop is the loop of the commit before the bytes
    entries, its decode kernel states the gain of the endomorphism tests apart from the gain of moving to the device."""
    import ctypes
    import snark_amd
    import pairing_cases as P
    from oracle.fields import BLS12_381, BN254
    from snark_amd._binding import Lib, ProofRaw
    C = {"bls12_381": BLS12_381, "bn254": BN254}[curve_name]
    lib = Lib(lib_path) if lib_path else snark_amd.lib()
    ctx = lib.ctx_create(0)
    lib.ctx_set_policy(ctx, "PAIRING_DEVICE", 1)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    pvk = lib.vk_process(ctx, C.curve_id, vk)
    sz = lib.sizes(C.curve_id)
    wires = [lib.proof_to_bytes(C.curve_id, *p, True) for p in proofs]
    psize = len(wires[0])
    rows = []
    for n in sizes:
        blob = b"".join(wires[j % 8] for j in range(n))
        xs = b"".join(inputs[j % 8] for j in range(n))
        buf = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
        xbuf = (ctypes.c_uint8 * len(xs)).from_buffer_copy(xs)
        arr = (ProofRaw * n)()
        ok = (ctypes.c_uint8 * n)()
        base = ctypes.addressof(buf)
        t = {"loop": [], "loop_pvk": [], "bytes": [], "decode": []}

        def parent_path():
            t0 = time.perf_counter()
            for j in range(n):
                rc = lib.dll.ark355_proof_from_bytes(C.curve_id, base + j * psize, psize, 1, 1, ctypes.byref(arr[j]))
                assert rc == 0
            t1 = time.perf_counter()
            assert lib.dll.ark355_verify_each_pvk(ctx, pvk, arr, xbuf, n, ok) == 0
            t2 = time.perf_counter()
            assert bytes(ok) == bytes([1]) * n
            return (t1 - t0) * 1e3, (t2 - t0) * 1e3

        def new_entry():
            t0 = time.perf_counter()
            got = lib.verify_each_bytes(ctx, pvk, blob, n, xs, True, 1)
            dt = (time.perf_counter() - t0) * 1e3
            assert got == ([True] * n, [0] * n)
            return dt

        def decode_stage():
            t0 = time.perf_counter()
            _, st = lib.proofs_from_bytes(ctx, C.curve_id, blob, n, sz, True, 1)
            dt = (time.perf_counter() - t0) * 1e3
            assert st == [0] * n
            return dt

        new_entry()
        decode_stage()                                  # warm-up: buffers allocated, code objects loaded
        for rep in range(reps):
            if n <= host_max and rep < 2:               # seconds per run: two runs state its spread
                a, b = parent_path()
                t["loop"].append(a)
                t["loop_pvk"].append(b)
            t["bytes"].append(new_entry())
            t["decode"].append(decode_stage())
        rows.append((n, t))
    lib.pvk_free(pvk)
    lib.ctx_destroy(ctx)
    print("curve %s, library %s: ms per call over %d interleaved runs (host clock), compressed proofs, VALIDATE_FULL"
          % (C.name, lib_path or "as built", reps))
    print("%7s | %14s %14s | %17s %19s | %17s | %8s"
          % ("proofs", "host loop", "loop + each_pvk", "verify_each_bytes", "(min .. max)", "proofs_from_bytes", "speed-up"))
    nan = float("nan")
    for n, t in rows:
        lp = statistics.median(t["loop"]) if t["loop"] else nan
        lv = statistics.median(t["loop_pvk"]) if t["loop_pvk"] else nan
        vb = statistics.median(t["bytes"])
        print("%7d | %14.3f %14.3f | %17.3f %19s | %17.3f | %8.2f"
              % (n, lp, lv, vb, "(%.3f .. %.3f)" % (min(t["bytes"]), max(t["bytes"])), statistics.median(t["decode"]), lv / vb))
    print("", flush=True)


def one_verify_each(count):
    """one ark355_verify_each of `count` BLS12-381 proofs on the device route, in this process (for a kernel trace)"""
    import snark_amd
    import pairing_cases as P
    from oracle.fields import BLS12_381 as C
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    lib.ctx_set_policy(ctx, "PAIRING_DEVICE", 1)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    ps = [proofs[j % 8] for j in range(count)]
    xs = b"".join(inputs[j % 8] for j in range(count))
    ok = lib.verify_each(ctx, C.curve_id, vk, ps, xs)
    lib.ctx_destroy(ctx)
    print("verify_each of %d proofs: %d accepted" % (count, sum(ok)))
    return 0 if all(ok) else 1


def one_verify(count):
    """one ark355_verify_batch of `count` BLS12-381 proofs under the default policy, in this process (for a kernel trace)"""
    import snark_amd
    import pairing_cases as P
    from oracle import serialize as Z
    from oracle.fields import BLS12_381 as C
    lib = snark_amd.lib()
    ctx = lib.ctx_create(0)
    vk, proofs, inputs, _, _ = P.oracle_batch(C, 8)
    rnd = random.Random(73)
    ps = [proofs[j % 8] for j in range(count)]
    xs = b"".join(inputs[j % 8] for j in range(count))
    rho = [Z.fr_canon(C, rnd.randrange(1, 1 << 128)) for _ in range(count)]
    ok = lib.verify_batch(ctx, C.curve_id, vk, ps, xs, rho if count > 1 else None)
    lib.ctx_destroy(ctx)
    print("verify_batch of %d proofs: %s" % (count, "accepted" if ok else "REJECTED"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per curve")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--one-verify", type=int, default=0, metavar="COUNT")
    ap.add_argument("--each", action="store_true", help="the per-group entries: pairing_groups(n, 1) and verify_each(n)")
    ap.add_argument("--host-max", type=int, default=1024, help="--each: largest n the host route is run at")
    ap.add_argument("--one-verify-each", type=int, default=0, metavar="COUNT")
    ap.add_argument("--pvk", action="store_true", help="verify_each against verify_each_pvk and vk_process")
    ap.add_argument("--from-bytes", action="store_true",
                    help="proofs as wire bytes: proof_from_bytes loop + verify_each_pvk against verify_each_bytes, and the decode stage")
    ap.add_argument("--lib", default=None, help="--from-bytes: another build of the library (path of the shared object)")
    a = ap.parse_args()
    if a.one_verify:
        return one_verify(a.one_verify)
    if a.one_verify_each:
        return one_verify_each(a.one_verify_each)
    if a.each and a.sizes == ",".join(str(s) for s in SIZES):
        a.sizes = ",".join(str(s) for s in EACH_SIZES)
    if a.pvk and a.sizes == ",".join(str(s) for s in SIZES):
        a.sizes = ",".join(str(s) for s in PVK_SIZES)
    if a.from_bytes and a.sizes == ",".join(str(s) for s in SIZES):
        a.sizes = "4096,65536"
        if a.host_max == 1024:
            a.host_max = 4096
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child:
        if a.from_bytes:
            child_bytes(a.child, a.reps, sizes, a.host_max, a.lib)
        elif a.pvk:
            child_pvk(a.child, a.reps, sizes)
        elif a.each:
            child_each(a.child, a.reps, sizes, a.host_max)
        else:
            child(a.child, a.reps, sizes)
        return 0
    text = []
    rc = 0
    for curve in a.curves.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", curve,
               "--reps", str(a.reps), "--sizes", a.sizes]
        if a.each:
            cmd += ["--each", "--host-max", str(a.host_max)]
        if a.pvk:
            cmd += ["--pvk"]
        if a.from_bytes:
            cmd += ["--from-bytes", "--host-max", str(a.host_max)] + (["--lib", a.lib] if a.lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        text.append(r.stdout)
        if r.returncode != 0:            # a fault, an abort or the time limit: nothing more is started on the device
            print("child for %s ended with status %d\n%s" % (curve, r.returncode, r.stderr[-2000:]), flush=True)
            rc = r.returncode
            break
    if a.out and rc == 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            if a.from_bytes:
                f.write("pairing_bench --from-bytes: proofs from wire bytes, one process per curve\n\n")
            elif a.pvk:
                f.write("pairing_bench --pvk: ark355_verify_each against ark355_verify_each_pvk on one handle, one process per curve\n\n")
            else:
                f.write("pairing_bench%s: host route (PAIRING_DEVICE=0) against device route (PAIRING_DEVICE=1), one process per curve\n\n"
                        % (" --each" if a.each else ""))
            f.write("".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
