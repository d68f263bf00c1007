"""The LDS layouts of the clearance kernels (csrc/clearance_lds.hpp, and the certified kernel's in csrc/clearance_cert.hpp): a kernel carves its LDS
with the function its launch sizes it with, so both are checked on the CPU by a small C++ program (tests/host/clearance_lds_check.cpp) under the
address and undefined-behaviour sanitizers — the byte count against the formulas the kernels were launched with before the carves existed, over
every table size the ceilings range over, and the arrays of a carve inside that count, apart and aligned."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clearance_lds_layouts(tmp_path):
    exe = str(tmp_path / "clearance_lds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "clearance_lds_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) > 30000, out.stdout
