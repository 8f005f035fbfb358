"""Host check of csrc/pipe_probe.h, the pipe kernel's count-form boundary
probe: the header is compiled into a stand-alone
program (tests/pipe_probe_check.cpp) with the system C++ compiler and run
over every sorted timestamp array of length 0..6 from a small value set, every
hint from -3 to n+3 and every seek around the values, against
std::upper_bound.  The program is built twice: plain, and with
-fsanitize=address,undefined (a stand-alone executable, nothing preloaded),
where each slab is a heap block of exactly the records the probe may read.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "victoriametrics_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_pipe_probe(tmp_path, sanitize):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "pipe_probe_check")
    cmd = [cxx, "-O1" if sanitize else "-O2", "-std=c++17", "-Wall", "-I", CSRC,
           os.path.join(HERE, "pipe_probe_check.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1] == "mismatches 0", r.stdout + r.stderr
    assert r.returncode == 0
