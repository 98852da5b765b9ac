"""CPU tier: the lane-pair Fq2 arithmetic of the G2 bucket accumulation on an emulated lane pair
(tests/cpp/test_g2_pair_emul.cpp, built with -DARK_EMUL so that every limb / column bound traps)."""
import os
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CPP_DIR = os.path.join(ROOT, "tests", "cpp")


def test_g2_pair_ops_and_chains_match_fq2():
    """Pair28::mul / sqr / mul2 and the "both components" operand forms against the single-lane Fq2 reference (random, 0, 1,
    -1, p - 1, top-of-class operands; both curves), then madd28_g2z chains with P + P, P - P, bases at infinity, openings and
    negated digits through ZzRegs and ZzLds."""
    src = os.path.join(CPP_DIR, "test_g2_pair_emul.cpp")
    exe = os.path.join(CPP_DIR, "test_g2_pair_emul")
    emul = os.path.join(ROOT, "tests", "emul")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DARK_EMUL", "-w", "-I", emul,
                           "-I", os.path.join(ROOT, "snark_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           src, os.path.join(emul, "hip_emul.cpp"), "-o", exe, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "g2 pair: all cases agree" in out.stdout
