"""Host check of csrc/vm_div1e3.h, the division-free `x / 1e3` the rate
evaluator uses for 31-bit dt: the header is compiled into a stand-alone
program (tests/div1e3_check.cpp) with the system C++ compiler and compared
with a true division for every integer x in [0, 2^32) and its negation.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "victoriametrics_amd", "csrc")


def test_div1e3_exhaustive(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "div1e3_check")
    # -ffp-contract=off as in the engine build: only the header's explicit
    # fma calls fuse.  -march=native turns them into one instruction on any
    # host with hardware FMA (about 2 s on 8 threads); where the compiler
    # does not take the flag, or the CPU has no FMA, they are libm calls
    # with the same results and the run takes a few times longer.
    base = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
            "-I", CSRC, os.path.join(HERE, "div1e3_check.cpp"), "-o", exe]
    if subprocess.run(base[:1] + ["-march=native"] + base[1:]).returncode:
        subprocess.run(base, check=True)
    threads = max(1, min(16, os.cpu_count() or 1))
    r = subprocess.run([exe, str(threads)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.stdout.strip() == "mismatches 0", r.stdout + r.stderr
    assert r.returncode == 0
