"""CPU-side checks of the product library: it loads, exports every symbol include/mpcmp.h declares, its host
logic (config, model, URDF reader, structure) agrees with the oracle, and compute calls fail loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def test_library_exports_every_declared_symbol(M):
    hdr = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    declared = set(re.findall(r"\b(mpcmp_[a-z_0-9]+)\s*\(", hdr))
    from mpc_motion_planner_amd import capi
    assert declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    lib = M.lib()
    for s in declared:
        assert hasattr(lib, s), s
    assert M.lib().mpcmp_version().startswith(b"mpcmp")


def _declarations():
    """every function include/mpcmp.h declares, in its order: (name, return type, argument kinds); an argument that is none of pointer, int,
    double, long gets the kind "?" """
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp.h")).read(), flags=re.S)
    out = []
    for ret, name, args in re.findall(r"\b(int|const\s+char\s*\*)\s*(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            if a != "void":
                kinds += "p" if "*" in a else {"int": "i", "double": "d", "long": "l"}.get(a.split(" ")[0] if re.fullmatch(r"\w+ \w+", a) else "", "?")
        out.append((name, "int" if ret == "int" else "text", kinds))
    return out


def test_abi_table_matches_the_header_and_the_library(M):
    """capi.ABI, the one table lib() declares to ctypes, against the header: the same functions in the same order, for each the exact argument
    kinds, and on the loaded library the exact argtypes and restype"""
    from mpc_motion_planner_amd import capi
    decl = _declarations()
    assert len(decl) == 84 and [d[0] for d in decl] == capi.SYMBOLS == list(capi.ABI)
    ctype = {"p": C.c_void_p, "i": C.c_int, "d": C.c_double, "l": C.c_long}
    for name, ret, kinds in decl:
        assert "?" not in kinds, (name, kinds)
        assert kinds == capi.ABI[name], (name, kinds, capi.ABI[name])
        f = getattr(M.lib(), name)
        assert f.argtypes == [ctype[k] for k in kinds], name
        assert f.restype is (C.c_char_p if ret == "text" else C.c_int), name
    assert [d[0] for d in decl if d[1] == "text"] == ["mpcmp_version", "mpcmp_last_error"]
    # the kinds the table had to learn beside int and pointer are in use
    assert capi.ABI["mpcmp_rh_run"] == "pidi" and capi.ABI["mpcmp_debug_fetch"] == "pipl" and capi.ABI["mpcmp_set_min_height"] == "pd"


def test_struct_layouts_match_header(M, tmp_path):
    assert C.sizeof(M.Info) == 64 and M.INFO_DTYPE.itemsize == 64
    assert C.sizeof(M.Config) == C.sizeof(o.Config) and C.sizeof(M.Model) == C.sizeof(o.Model)
    # the header itself, through a C compiler: sizes and the offsets of the fields appended last
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mpcmp_config), '
                   'sizeof(mpcmp_model), sizeof(mpcmp_info), offsetof(mpcmp_config, qp_warm_start), offsetof(mpcmp_config, lbT)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sz == [C.sizeof(M.Config), C.sizeof(M.Model), C.sizeof(M.Info), M.Config.qp_warm_start.offset, M.Config.lbT.offset], sz


def test_config_and_limits_match_oracle(M):
    for margins in [(1, 1, 1, 1), (0.9, 0.9, 0.5, 0.9), (0.8, 0.8, 0.6, 0.9)]:
        a = M.default_config(4, 20, margins=margins); b = o.default_config(4, 20, margins=margins)
        assert bytes(a) == bytes(b)
    la, lb = M.default_limits(), o.default_limits()
    for k in la:
        assert np.array_equal(la[k], lb[k])
    # set_constraint_margins arithmetic (motionPlanner.cpp:66-75)
    c = M.default_config(4, 2, margins=(0.9, 0.9, 0.5, 0.9))
    s = 0.1 * (2.8973 + 2.8973) / 2
    assert abs(c.lbx[0] - (-2.8973 + s)) < 1e-15 and abs(c.ubx[7] - 0.9 * 2.175) < 1e-15
    assert abs(c.ubu[1] - 0.5 * 7.5) < 1e-15 and abs(c.ubg[4] - 0.9 * 12) < 1e-15 and c.lbg[7] == 0.05 and np.isinf(c.ubg[7])


def test_model_matches_oracle_and_urdf(M):
    a, b = M.default_model(), o.default_model()
    for f in ["R0", "p", "mass", "com", "I", "tool", "link8", "gravity"]:
        assert np.array_equal(np.array(getattr(a, f)), np.array(getattr(b, f))), f
    u = M.model_from_urdf(os.path.join(ROOT, "tests", "golden", "panda_arm.urdf"))      # the Panda description the model was taken from
    for f in ["R0", "p", "mass", "com", "I", "tool", "link8", "gravity"]:
        assert np.array_equal(np.array(getattr(a, f)), np.array(getattr(u, f))), f
    assert abs(u.mass[6] - 1.735522) < 1e-12      # link7 + link8 (m=0) + tool (m=1) lumped


def test_urdf_reader_rejects_bad_input(M, tmp_path):
    with pytest.raises(M.MpcmpError):
        M.model_from_urdf(str(tmp_path / "missing.urdf"))
    p = tmp_path / "two_joints.urdf"
    p.write_text('<robot name="x"><link name="a"/><link name="b"/><joint name="j" type="revolute"><parent link="a"/>'
                 '<child link="b"/><axis xyz="0 0 1"/></joint></robot>')
    with pytest.raises(M.MpcmpError):
        M.model_from_urdf(str(p))


def test_time_nodes_and_dims(M):
    for ns in (1, 2, 4, 6, 8):
        assert M.num_nodes(ns) == 3 * ns + 1
        assert np.array_equal(M.time_nodes(ns), o.time_nodes(ns))


def test_scenarios_are_seeded_and_feasible(M):
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(64)
    x0b, xfb = scenarios.make_batch(64)
    assert np.array_equal(x0, x0b) and np.array_equal(xf, xfb)
    x0c, _ = scenarios.make_batch(32, stream_offset=32)
    assert np.array_equal(x0c, x0[32:])            # shard r of the global batch == its slice (multi-GPU sharding)
    cfg = M.default_config(4, 2, margins=(0.9, 0.9, 0.5, 0.9))
    for x in (x0, xf):
        assert np.all(x[:, :7] >= np.array(cfg.lbx[:7]) - 1e-12) and np.all(x[:, :7] <= np.array(cfg.ubx[:7]) + 1e-12)
        assert np.all(np.abs(x[:, 7:]) <= np.array(cfg.ubx[7:]) + 1e-12)
        # rejection rule of sample_random_state: joint-7 origin above min_height (motionPlanner.cpp:111)
        assert np.all(scenarios.joint7_height(M.default_model(), x[:, :7]) >= 0.05)
        for i in range(8):
            assert abs(scenarios.joint7_height(M.default_model(), x[i:i + 1, :7])[0] - o.fk(x[i, :7])[0][2]) < 1e-12


def test_no_cpu_fallback(M):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = M.default_config(4, 2)
    with pytest.raises(M.MpcmpError) as e:
        M.Solver(cfg, 4)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_bad_config_rejected_before_touching_the_gpu(M):
    ctx = C.c_void_p()
    bad = M.default_config(3, 2)
    assert M.lib().mpcmp_create(C.byref(bad), None, 0, 4, C.byref(ctx)) == -1
    good = M.default_config(4, 2)
    assert M.lib().mpcmp_create(C.byref(good), None, 0, 0, C.byref(ctx)) == -1
    assert M.lib().mpcmp_create(None, None, 0, 4, C.byref(ctx)) == -1


def _edit(c, field, v):
    """field: a name, or (name, index) of a bound table entry"""
    if isinstance(field, tuple):
        getattr(c, field[0])[field[1]] = v
    else:
        setattr(c, field, v)


NAN, INF = float("nan"), float("inf")
# (field, a value no kernel or oracle gives a meaning to, a valid value of the same field)
BAD_SETTINGS = [("eps_abs", NAN, 0.0), ("eps_abs", -1e-3, 0.0), ("eps_rel", NAN, 0.0), ("eps_rel", -1e-6, 0.0), ("eps_target", NAN, 0.0),
                ("eps_target", -1e-2, 0.0), ("hess_reg", NAN, 0.0), ("hess_reg", -1e-3, 0.0), ("rho_eq_scale", 0.0, 1.0), ("rho_eq_scale", -1e3, 1.0),
                ("rho_eq_scale", NAN, 1.0), ("ls_eta", 0.0, 0.1), ("ls_eta", 1.0, 0.9), ("ls_eta", NAN, 0.25), ("ls_tau", 0.0, 0.7), ("ls_tau", 1.0, 0.7),
                ("ls_tau", -0.5, 0.5), ("ls_tau", NAN, 0.5), ("quirk_dtau_dT", 2, 0), ("quirk_dtau_dT", -1, 1),
                (("lbx", 3), 5.0, -INF), (("ubx", 9), NAN, INF), (("lbx", 0), NAN, 0.25), (("lbu", 2), 1e9, -INF), (("ubu", 6), NAN, 0.0),
                (("lbg", 4), 1e3, -INF), (("ubg", 0), -1e3, INF), (("lbg", 7), NAN, -INF), (("ubg", 7), NAN, INF), (("lbg", 7), INF, 0.05),
                (("ubx", 1), -INF, INF), ("lbT", 11.0, 0.0), ("ubT", NAN, INF), ("lbT", NAN, -INF), ("ubT", -1.0, 10.0)]


@pytest.mark.parametrize("field,bad,good", BAD_SETTINGS, ids=["%s=%s" % (f if isinstance(f, str) else "%s[%d]" % f, b) for f, b, _ in BAD_SETTINGS])
def test_meaningless_settings_rejected_before_touching_the_gpu(M, field, bad, good):
    """validate() runs before mpcmp_create looks for a device: a meaningless setting (NaN, a negative tolerance or shift, rho_eq_scale <= 0, a line
    search fraction outside (0, 1), quirk_dtau_dT not 0 / 1, lb > ub, NaN or an empty box in any bound) is MPCMP_EINVAL with a message, for one arm
    and two; the same configuration with a valid value (infinite bound ends included) passes validation: -2 without a GPU (0 with one)"""
    import torch
    gpu = torch.cuda.is_available()
    models = M.arm_models(M.DUAL_BASES)
    for narm in (1, 2):
        c = M.default_config(6, 2, margins=(0.9, 0.9, 0.5, 0.9))
        _edit(c, field, bad)
        ctx = C.c_void_p()
        rc = M.lib().mpcmp_create(C.byref(c), None, 0, 1, C.byref(ctx)) if narm == 1 else M.lib().mpcmp_create_multi(C.byref(c), models, 2, 0, 1, C.byref(ctx))
        assert rc == -1 and not ctx.value, (narm, field, bad, rc)
        assert M.lib().mpcmp_last_error(None), (narm, field, bad)
        _edit(c, field, good)
        rc = M.lib().mpcmp_create(C.byref(c), None, 0, 1, C.byref(ctx)) if narm == 1 else M.lib().mpcmp_create_multi(C.byref(c), models, 2, 0, 1, C.byref(ctx))
        assert rc == (0 if gpu else -2), (narm, field, good, rc, M.lib().mpcmp_last_error(None))
        if ctx.value:
            M.lib().mpcmp_destroy(ctx)


def test_narrow_general_rows_rejected_below_num_seg_6(M):
    """a general row narrower than 1e-4 (rho_eq in the oracle) is EINVAL for num_seg 1, 2, 4 (k_qp / k_qp2 assemble every general row with the
    plain rho); num_seg 6 and 8 take it, and a row of 2e-4 passes everywhere"""
    import torch
    gpu = torch.cuda.is_available()
    for nseg in (1, 2, 4, 6, 8):
        for q, w in ((2, 5e-5), (7, 0.0), (2, 2e-4)):
            c = M.default_config(nseg, 2, margins=(0.9, 0.9, 0.5, 0.9))
            c.lbg[q], c.ubg[q] = 0.05 - w / 2, 0.05 + w / 2
            ctx = C.c_void_p()
            rc = M.lib().mpcmp_create(C.byref(c), None, 0, 1, C.byref(ctx))
            assert rc == (-1 if nseg <= 4 and w < 1e-4 else (0 if gpu else -2)), (nseg, q, w, rc)
            if rc == -1:
                assert b"lbg" in M.lib().mpcmp_last_error(None)
            if ctx.value:
                M.lib().mpcmp_destroy(ctx)


def test_cpp_shim_and_example_compile(M, tmp_path):
    """the header-only MotionPlanner mirror and the offline_trajectory counterpart build with plain g++"""
    exe = str(tmp_path / "offline_trajectory")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "offline_trajectory.cpp"),
                           "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe])
    # the selftest touches every member of the mirror, incl. the write side of `mpc` and the Ruckig look-alikes (-Wall -Werror:
    # the header must stay warning-free for a caller's build)
    exe2 = str(tmp_path / "shim_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "shim_selftest.cpp"),
                           "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe2])
    import torch
    if not torch.cuda.is_available():
        for e in (exe, exe2):
            r = subprocess.run([e], capture_output=True, text=True)
            assert r.returncode == 1 and "no CPU fallback" in r.stderr


# ---- scenario helpers of the robot wrapper (robot_utils/pandaWrapper.cpp:14-107): host code, no GPU needed ----
def _rand_q(rng, M):
    lim = M.default_limits()
    return lim["qmin"] + (lim["qmax"] - lim["qmin"]) * (0.15 + 0.7 * rng.random(7))


def test_tool_jacobian_and_forward_velocities_match_oracle(M):
    rng = np.random.default_rng(7)
    mdl, omdl = M.default_model(), o.default_model()
    for _ in range(20):
        q, qd = _rand_q(rng, M), rng.normal(size=7)
        J, p, R = M.tool_jacobian(mdl, q)
        Jo = o.frame_jacobian(q, np.array(omdl.tool), omdl)
        p7, R7, p8, pt = o.fk(q, omdl)
        assert np.abs(J - Jo).max() < 1e-12 and np.abs(p - pt).max() < 1e-12 and np.abs(R - R7).max() < 1e-12
        assert np.abs(M.forward_velocities(mdl, q, qd) - Jo @ qd).max() < 1e-12
        # the linear rows are the derivative of the tool position (central differences)
        for j in range(7):
            e = np.zeros(7); e[j] = 1e-6
            dp = (M.tool_jacobian(mdl, q + e)[1] - M.tool_jacobian(mdl, q - e)[1]) / 2e-6
            assert np.abs(dp - J[:3, j]).max() < 1e-8


def test_inverse_velocities_is_the_damped_pseudo_inverse(M):
    rng = np.random.default_rng(8)
    mdl = M.default_model()
    for _ in range(20):
        q = _rand_q(rng, M)
        lin, ang = rng.uniform(-1.7, 1.7, 3), np.zeros(3)          # examples/benchmark.cpp:20: zero angular speed
        J = M.tool_jacobian(mdl, q)[0]
        qd = M.inverse_velocities(mdl, q, lin, ang)
        ref = J.T @ np.linalg.solve(J @ J.T + 1e-5 * np.eye(6), np.concatenate([lin, ang]))
        assert np.abs(qd - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
        back = M.forward_velocities(mdl, q, qd)
        if np.linalg.cond(J @ J.T) < 1e3:                          # away from singularities the damping is negligible
            assert np.abs(back - np.concatenate([lin, ang])).max() < 1e-2


def test_inverse_kinematic_reaches_reachable_poses(M):
    rng = np.random.default_rng(9)
    mdl = M.default_model()
    ok = 0
    for _ in range(10):
        q_true = _rand_q(rng, M)
        _, p, R = M.tool_jacobian(mdl, q_true)
        q, conv, it = M.inverse_kinematic(mdl, R, p, q_init=q_true + 0.3 * rng.normal(size=7))
        _, p2, R2 = M.tool_jacobian(mdl, q)
        if conv:
            ok += 1
            assert it <= 1000 and np.abs(p2 - p).max() < 2e-4 and np.abs(R2 - R).max() < 2e-4
    assert ok >= 8
    # an unreachable pose hits the iteration cap and says so
    q, conv, it = M.inverse_kinematic(mdl, np.eye(3), np.array([3.0, 0.0, 0.0]))
    assert not conv and it == 1000


def _build_inputs(csrc):
    """the files of csrc/ a build reads: everything but build products and hidden files"""
    skip = (".o", ".so", ".a", ".bc", ".hipi")
    return sorted(f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f)) and not f.startswith(".") and not f.endswith(skip)
                  and "-hip-amdgcn-" not in f and "-host-x86_64-" not in f)


def test_every_source_file_is_a_build_dependency(M):
    """build_library() rebuilds when any file the library is built from is newer than the library: every file of csrc/ (sources, headers of every
    translation unit, the Makefile with its per-unit compiler options) and the public header"""
    from mpc_motion_planner_amd import capi
    csrc = os.path.join(ROOT, "mpc_motion_planner_amd", "csrc")
    deps = {os.path.realpath(d) for d in capi.build_dependencies()}
    files = _build_inputs(csrc)
    assert {"qp3_n25.hip", "qp5_n19.hip", "Makefile", "mpcmp.hip", "solver.hip", "model_host.cpp"} <= set(files)
    missing = [f for f in files if os.path.realpath(os.path.join(csrc, f)) not in deps]
    assert not missing, missing
    assert os.path.realpath(os.path.join(ROOT, "include", "mpcmp.h")) in deps
    assert all(os.path.isfile(d) for d in deps)


def test_build_library_rebuilds_after_an_edit_to_any_source(M, tmp_path, monkeypatch):
    """a copy of the sources with a library newer than all of them: no rebuild; then each file in turn made newer than the library (an edit to
    qp5_n19.hip among them): build_library() runs make in that source directory"""
    import shutil
    from mpc_motion_planner_amd import capi
    csrc = os.path.join(ROOT, "mpc_motion_planner_amd", "csrc")
    pkg = tmp_path / "mpc_motion_planner_amd"
    (pkg / "csrc").mkdir(parents=True); (tmp_path / "include").mkdir()
    files = _build_inputs(csrc)
    for f in files:
        shutil.copy(os.path.join(csrc, f), pkg / "csrc" / f)
    shutil.copy(os.path.join(ROOT, "include", "mpcmp.h"), tmp_path / "include" / "mpcmp.h")
    so = pkg / "libmpcmp.so"
    so.write_bytes(b"")
    t0 = 1.0e9
    for p in [pkg / "csrc" / f for f in files] + [tmp_path / "include" / "mpcmp.h"]:
        os.utime(p, (t0, t0))
    os.utime(so, (t0 + 10, t0 + 10))
    calls = []
    monkeypatch.setattr(capi, "_HERE", str(pkg))
    monkeypatch.setattr(capi, "_SO", str(so))
    monkeypatch.setattr(capi.subprocess, "check_call", lambda cmd, **kw: calls.append(list(cmd)))
    capi.build_library()
    assert calls == []                                         # up to date
    for i, p in enumerate([pkg / "csrc" / "qp5_n19.hip"] + [pkg / "csrc" / f for f in files] + [tmp_path / "include" / "mpcmp.h"]):
        os.utime(p, (t0 + 20 + 2 * i, t0 + 20 + 2 * i))              # an edit after the last build
        del calls[:]
        capi.build_library()
        assert len(calls) == 1 and calls[0][:3] == ["make", "-C", str(pkg / "csrc")], (p, calls)
        os.utime(so, (t0 + 21 + 2 * i, t0 + 21 + 2 * i))             # (the rebuilt library)
        del calls[:]
        capi.build_library()
        assert calls == [], p
