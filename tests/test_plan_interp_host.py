"""The node interpolant every reader of a finished plan shares (csrc/plan_interp.hpp): host and device run one source, so it is checked on the CPU by
a small C++ program (tests/host/plan_interp_check.cpp) — the ends and the interior boundaries exactly, the clamp and the extrapolation outside
[0, 1], the sum of the weights, the node times of mpcmp_time_nodes, and cubics reproduced between the nodes, each within a bound derived there."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_interp(tmp_path):
    exe = str(tmp_path / "plan_interp_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "plan_interp_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for nseg in (1, 2, 4, 6, 8):
        assert "ok %d\n" % nseg in out.stdout
