"""Host-only unit test of the prover's schedule plan (snark_amd/csrc/prove_plan.h; tests/cpp/test_prove_plan.cpp): every stream role
and schedule decision of a proof over the whole input space, against the rules that prove_run's comments state -- the emulator
runs every stream as one and never has a second proof in flight, so the CPU tier sees none of them otherwise."""
import os
import subprocess

from conftest import ROOT


def test_prove_plan_rules(tmp_path):
    exe = str(tmp_path / "test_prove_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "snark_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_prove_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.stdout, out.stderr)
