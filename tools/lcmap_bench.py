#!/usr/bin/env python3
"""finalize() on the device against the host route, both curves: builds tools/lcmap_host_route.cpp against
the library and runs it on
  bench   the 2^20-constraint system of relations/examples/bench.rs:22-83 (depth 1)
  deep    2^18 rows in chains of 32 running sums (depth 31), the shape field-gadget additions produce
with 20 interleaved repeats; every line gives the median, the minimum and max - min of the host clock.  (dev) is
ark355_gr1cs_from_lcs from host arrays, upload and handle construction included; (host) is what a host has without it: the C++
mirror's inline_all_lcs + to_matrices on one thread, the rows flattened to CSR, ark355_gr1cs_load.  Per-kernel times come from a
`rocprofv3 --kernel-trace --stats` run of the built program itself (profiles/README.md).
Dev tool; run on an MI355X:  python tools/lcmap_bench.py [--reps 20] [--out profiles/lcmap_bench.txt]"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SRC = os.path.join(ROOT, "tools", "lcmap_host_route.cpp")
EXE = os.path.join(ROOT, "tools", "lcmap_host_route.bin")


def build(libdir=None, libname="ark355"):
    """the program next to its source; rebuilt when the source, the mirror or the header is newer"""
    libdir = libdir or os.path.join(ROOT, "snark_amd")
    deps = [SRC, os.path.join(ROOT, "include", "ark355.h")] + [os.path.join(ROOT, "host_mirror", f) for f in ("relations.hpp", "snark.hpp")]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", SRC, "-o", EXE, "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir])
    return EXE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--circuits", default="bench:20,deep:18", help="name:log2(rows), comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    exe = build()
    lines = ["lcmap_bench: %d interleaved repeats after %d warm-up rounds; ms per call (host clock)" % (a.reps, a.warmup)]
    print(lines[0], flush=True)
    for curve in a.curves.split(","):
        for spec in a.circuits.split(","):
            name, log_n = spec.split(":")
            out = subprocess.run([exe, curve, name, log_n, str(a.reps), str(a.warmup)], capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit("lcmap_host_route %s %s failed (%d): %s" % (curve, spec, out.returncode, out.stderr[-2000:]))
            print(out.stdout, end="", flush=True)
            lines += out.stdout.splitlines()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
