"""CPU-side checks of the batched tool-pose targets (mpcmp_pose_targets_batch[_device], include/mpcmp.h): the ABI, the host inverse
kinematics the kernel shares its DLS step with (pinned bit for bit by a fixture of the library before that refactor), the seeded starts
of scenarios.ik_seeds, and the register / scratch budget of the kernel (hipcc cross-compiles for gfx950: no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_motion_planner_amd", "csrc")

# k_pose_targets as the product flags compile it: 256 VGPRs (+ 22 AGPRs the allocator parks values in), one wave per SIMD, no scratch
IK_VGPRS, IK_MAX_AGPRS = 256, 32


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def test_header_declares_pose_targets_and_library_exports_them(M):
    hdr = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    for name in ("mpcmp_pose_targets_batch", "mpcmp_pose_targets_batch_device"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(M.lib(), name), name
    assert "} mpcmp_ik_info;" in hdr
    for name, v in (("MPCMP_IK_NOT_CONVERGED", M.IK_NOT_CONVERGED), ("MPCMP_IK_Q_OUT_OF_BOUNDS", M.IK_Q_OUT_OF_BOUNDS),
                    ("MPCMP_IK_QD_OUT_OF_BOUNDS", M.IK_QD_OUT_OF_BOUNDS)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), hdr), name


def test_ik_info_layout_matches_header(M, tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(mpcmp_ik_info), offsetof(mpcmp_ik_info, err), offsetof(mpcmp_ik_info, seed), offsetof(mpcmp_ik_info, iters), '
                   'offsetof(mpcmp_ik_info, status), offsetof(mpcmp_ik_info, pad)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    d = M.IK_INFO_DTYPE
    assert got == [d.itemsize] + [d.fields[f][1] for f in ("err", "seed", "iters", "status", "pad")], got


def test_host_inverse_kinematics_matches_fixture(M):
    """mpcmp_inverse_kinematics now runs the DLS step shared with the kernel; its results are those of the library before, bit for bit"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ik_host_ref.npz"))
    model = M.default_model()
    assert len(g["p"]) == 64 and g["rc"][-1] == 1 and g["iters"][-1] == 1000        # the last pose is out of reach
    for i in range(len(g["p"])):
        q, ok, it = M.inverse_kinematic(model, g["R"][i], g["p"][i], g["q_init"][i])
        assert np.array_equal(q, g["q"][i]), (i, q - g["q"][i])
        assert it == g["iters"][i] and (0 if ok else 1) == g["rc"][i], i


def test_ik_seeds_seeded_in_bounds_and_per_stream(M):
    from mpc_motion_planner_amd import scenarios
    cfg = M.default_config(4, 3, margins=(0.9, 0.9, 0.5, 0.9, 0.1))
    lo, hi = np.array(cfg.lbx[:7]), np.array(cfg.ubx[:7])
    a = scenarios.ik_seeds(64, 16, cfg)
    assert a.shape == (64, 16, 7) and a.dtype == np.float64
    assert np.array_equal(a, scenarios.ik_seeds(64, 16, cfg))                   # reproducible
    assert (a >= lo).all() and (a <= hi).all()
    assert np.array_equal(a[:8], scenarios.ik_seeds(8, 16, cfg))                # problem i's starts do not depend on B
    assert not np.array_equal(a, scenarios.ik_seeds(64, 16, cfg, seed=scenarios.SEED + 1))
    # spread over the box, not a constant
    assert (a.reshape(-1, 7).std(axis=0) > 0.2 * (hi - lo)).all()
    # wider bounds (no margin) widen the draw
    full = scenarios.ik_seeds(64, 16, M.default_config(4, 3))
    assert full.min() < lo.min() or full.max() > hi.max()


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    fl = re.search(r"^FLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    return [f for f in fl if f not in ("-Wall", "-Wno-unused-function")]


def test_ik_kernel_compiles_without_scratch(tmp_path):
    src = tmp_path / "probe.hip"
    src.write_text('#include "ik_device.hpp"\n')
    cmd = ["/opt/rocm/bin/hipcc"] + _flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC,
                                                 "-c", "-o", str(tmp_path / "probe.o"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"\bAGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                res[cur][key] = int(m.group(1))
    k = [v for n, v in res.items() if n.startswith("_ZN5mpcmp14k_pose_targets")]
    assert len(k) == 1, res
    assert k[0]["scratch"] == 0, k[0]
    assert k[0]["vgpr"] == IK_VGPRS and k[0]["agpr"] <= IK_MAX_AGPRS, k[0]
