"""CPU tier: the emulator's allocator on its own (tests/cpp/test_alloc_emul.cpp): poisoned bodies, guard bands on both sides, a
damaged band reported once as an error that names the allocation -- and a process that lives to report it."""
import os
import subprocess

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CPP_DIR = os.path.join(ROOT, "tests", "cpp")


def test_poison_guard_bands_and_pending_error():
    src = os.path.join(CPP_DIR, "test_alloc_emul.cpp")
    exe = os.path.join(CPP_DIR, "test_alloc_emul")
    emul = os.path.join(ROOT, "tests", "emul")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-DARK_EMUL", "-w", "-I", emul, src, os.path.join(emul, "hip_emul.cpp"), "-o", exe, "-lpthread"]
    # a stand-alone host program: under the address sanitizer where the compiler ships one (the bands lie inside the block the
    # allocator took from the heap, so the stores of this test are legal and anything past the bands is the sanitizer's)
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    # (the emulator keeps its coroutine stacks for the life of the process: not a leak to report)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "emulator allocator: all cases agree" in out.stdout
