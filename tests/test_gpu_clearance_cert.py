"""Certified clearance on the GPU (mpcmp_clearance_certified_batch*, include/mpcmp_clearance_cert.h): the kernel against the host statement of the
rule on the cases of tests/test_clearance_cert_host.py (where the reference's decision gaps are asserted), independence of the batch, what the
sampled checker cannot see, and the way of the certified records through the selection, the route join, the façade and the C++ shim.

Bounds.  Integers equal, doubles within 1e-12 (1 + |x|), as between the host statement and the reference: kernel and host statement run one source,
the kernel with contracted multiply-adds and the device's sine and cosine.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import clearance_cert_reference as R
import test_clearance_cert_host as H

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
MARGIN = H.MARGIN
MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def solver(M, narm, nseg, max_batch, tables=None, obstacles=None):
    models, _, tabs = H.robot(narm)
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    for a, t in enumerate(tabs if tables is None else tables):
        s.set_robot_spheres(t, arm=a)
    if obstacles is not None:
        s.set_obstacles(obstacles)
    return s


# ---- 1. the kernel against the host statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm,nseg,self_gap,n_start,max_depth,seed", H.CASES)
def test_kernel_matches_host_statement(M, narm, nseg, self_gap, n_start, max_depth, seed):
    ref = H.case_reference(narm, nseg, self_gap, n_start, max_depth, seed)
    assert min(r["gap"] for r in ref) > H.GAP
    x, T = H.plans(narm, nseg, seed)
    s = solver(M, narm, nseg, x.shape[0], obstacles=H.world(narm))
    clr, cert = s.clearance_certified(x, T, MARGIN, self_gap, n_start, max_depth)
    for b in range(x.shape[0]):
        hc, ht = H.one(M, narm, nseg, H.world(narm), x[b], T[b], MARGIN, self_gap, n_start, max_depth)
        H.check_records(clr[b], cert[b], dict(clr=hc, cert=ht), ("host", narm, nseg, b))
        H.check_records(clr[b], cert[b], ref[b], ("reference", narm, nseg, b))
    # cert may be left out: the first record is the same
    only = np.zeros(x.shape[0], dtype=M.CLEARANCE_DTYPE)
    xc, Tc = np.ascontiguousarray(x), np.ascontiguousarray(T)
    assert M.lib().mpcmp_clearance_certified_batch(s._ctx, x.shape[0], xc.ctypes.data, Tc.ctypes.data, MARGIN, self_gap, n_start, max_depth,
                                                   only.ctypes.data, None) == 0
    assert only.tobytes() == clr.tobytes()


def test_capacity_rule_on_the_gpu(M):
    """the long graze of the host test at n0 = 4096: 2048 intervals split, the others undecided; and max_depth 16 on a hit deep in the tree"""
    _, arrays, _ = H.robot(1)
    nseg, n_start = 4, 1024
    q0 = np.array([-1.0, -0.5, 0.0, -2.0, 0.0, 1.6, 0.0]); q1 = q0.copy(); q1[0] = 1.0; q1[1] = -0.5 + 1e-5
    tau = M.time_nodes(nseg)
    x = np.zeros((1, tau.shape[0], 14)); x[0, :, :7] = q0[None] + (q1 - q0)[None] * tau[:, None]
    table = M.spheres([3], [[0.0, 0.0, 0.0]], 0.05)
    z = [R.frames(arrays[0], R.position(nseg, x[0], t))[1][3][2] for t in np.linspace(0.0, 1.0, 2001)]
    ob = np.array([M.obstacle(M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (min(z) - 0.05 - MARGIN - 1e-5, 0, 0), 0.0)], dtype=M.OBSTACLE_DTYPE)
    s = solver(M, 1, nseg, 2, tables=[table], obstacles=ob)
    clr, cert = s.clearance_certified(x, np.array([2.0]), MARGIN, 0, n_start, 1)
    hc, ht = H.one(M, 1, nseg, ob, x[0], 2.0, MARGIN, 0, n_start, 1, tables=[table])
    H.check_records(clr[0], cert[0], dict(clr=hc, cert=ht), "capacity")
    assert cert["n_eval"][0] == 8192 and cert["n_undecided"][0] == 2048 + 4096 and clr["status"][0] == M.CLR_UNDECIDED
    xt, T, tab, cap, _ = H.thin_capsule_case()
    s2 = solver(M, 1, 4, 2, tables=[tab], obstacles=cap)
    clr, cert = s2.clearance_certified(xt[None], np.array([T]), 0.0, 0, 1, 16)
    hc, ht = H.one(M, 1, 4, cap, xt, T, 0.0, 0, 1, 16, tables=[tab])
    H.check_records(clr[0], cert[0], dict(clr=hc, cert=ht), "depth 16")


# ---- 2. a plan's records do not depend on the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", [False, True])
def test_records_do_not_depend_on_the_batch(M, per_problem):
    x12, T12 = H.plans(1, 4, 15)
    idx = np.arange(33) % 12
    x, T = np.ascontiguousarray(x12[idx]), np.ascontiguousarray(T12[idx] * (1.0 + 0.01 * np.arange(33)))
    obs = H.world(1)
    if per_problem:
        obs = np.repeat(obs[None], 33, axis=0)
        obs["a"][:, 0, 2] += 0.01 * np.arange(33)                      # (the sphere obstacle of set b stands b cm higher)
    s = solver(M, 1, 4, 33, obstacles=obs)
    clr, cert = s.clearance_certified(x, T, MARGIN, 4, 4, 10)
    rev = slice(None, None, -1)
    if per_problem:
        s.set_obstacles(np.ascontiguousarray(obs[rev]))
    clr_r, cert_r = s.clearance_certified(np.ascontiguousarray(x[rev]), np.ascontiguousarray(T[rev]), MARGIN, 4, 4, 10)
    assert clr_r[rev].tobytes() == clr.tobytes() and cert_r[rev].tobytes() == cert.tobytes()
    for b in (0, 7, 20, 32):
        if per_problem:
            s.set_obstacles(np.ascontiguousarray(obs[b:b + 1]))
        c1, t1 = s.clearance_certified(x[b:b + 1], T[b:b + 1], MARGIN, 4, 4, 10)
        assert c1.tobytes() == clr[b:b + 1].tobytes() and t1.tobytes() == cert[b:b + 1].tobytes(), b
    assert len(set(clr["status"].tolist())) >= 2


# ---- 3. the motivating case --------------------------------------------------------------------------------------------------------------------
def test_a_crossing_between_samples_is_found(M):
    x, T, table, ob, ts = H.thin_capsule_case()
    s = solver(M, 1, 4, 4, tables=[table], obstacles=ob)
    sampled = s.clearance(x[None], np.array([T]), 20, 0.0, 0)
    assert sampled["status"][0] == 0 and sampled["d_min"][0] >= 0.0
    clr, cert = s.clearance_certified(x[None], np.array([T]), 0.0, 0, 4, 10)
    assert clr["status"][0] & M.CLR_HIT and clr["d_min"][0] < 0.0 and 7 / 20 * T < clr["t_min"][0] < 8 / 20 * T
    assert cert["d_lower"][0] <= clr["d_min"][0] and clr["sphere"][0] == 0 and clr["other"][0] == 0


# ---- 4. two arms: the wrists cross between samples -------------------------------------------------------------------------------------------
def two_arm_crossing(M):
    """Two arms facing each other 1 m apart hold the same planar posture whose tool point lies on the axis between the bases (x = 0.5, y = 0), so
    the two tool points coincide; arm 0 stays there, arm 1 swings its first joint from -0.3 to 0.5 rad and passes through that posture at
    sigma = 3/8, t = 0.43, between samples 8 and 9 of n_pts = 20.  One sphere of 3 mm per arm at the tool point."""
    models, arrays, _ = H.robot(2)
    tool = np.array(list(models[0].tool))

    def tool_x(q1):
        Rs, ps = R.frames(arrays[0], np.array([0.0, q1, 0.0, -2.0, 0.0, 2.2, 0.0]))
        return (ps[6] + Rs[6] @ tool)[0]
    lo, hi = -1.0, -0.5
    assert tool_x(lo) < 0.5 < tool_x(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tool_x(mid) < 0.5 else (lo, mid)
    qa = np.array([0.0, 0.5 * (lo + hi), 0.0, -2.0, 0.0, 2.2, 0.0])
    q0, q1 = np.concatenate([qa, qa]), np.concatenate([qa, qa])
    q0[7] = -0.3; q1[7] = 0.5
    tables = [M.spheres([6], [tool], 0.003), M.spheres([6], [tool], 0.003)]
    return H.swing(6, q0, q1), 2.0, tables


def test_two_arms_cross_between_samples(M):
    x, T, tables = two_arm_crossing(M)
    s = solver(M, 2, 6, 4, tables=tables)
    sampled = s.clearance(x[None], np.array([T]), 20, 0.0, 0)
    assert sampled["status"][0] == 0 and sampled["d_min"][0] > 0.0 and sampled["other"][0] == -2
    clr, cert = s.clearance_certified(x[None], np.array([T]), 0.0, 0, 4, 10)
    assert clr["status"][0] & M.CLR_HIT and clr["sphere"][0] == 0 and clr["other"][0] == -2 and clr["d_min"][0] < 0.0
    assert 8 / 20 * T < clr["t_min"][0] < 9 / 20 * T and 8 / 20 * T < clr["t_first"][0] < 9 / 20 * T
    hc, ht = M.clearance_certified_one(H.robot(2)[0], 6, tables, None, x, T, 0.0, 0, 4, 10)
    H.check_records(clr[0], cert[0], dict(clr=hc, cert=ht), "two arms")


# ---- 5. selection end to end ---------------------------------------------------------------------------------------------------------------------
def candidates(M):
    """two groups of three candidates in the world of the thin capsule: the fastest of each group crosses it between samples, the others swing
    with the second joint 0.4 rad and 0.8 rad further back and stay away from it"""
    x, _, table, ob, _ = H.thin_capsule_case()
    other = []
    for dq in (0.4, 0.8):
        a, b = np.array([-0.9, -0.4 - dq, 0.2, -2.0, 0.1, 1.8, 0.5]), np.array([1.1, -0.4 - dq, 0.2, -1.4, 0.1, 1.8, 0.5])
        other.append(H.swing(4, a, b))
    sx = np.ascontiguousarray(np.stack([x, other[0], other[1], other[1], x, other[0]]))
    sT = np.array([1.0, 1.5, 2.0, 1.8, 0.9, 1.2])
    group = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    return sx, sT, group, table, ob


def test_selection_takes_the_fastest_certified_candidate(M):
    sx, sT, group, table, ob = candidates(M)
    s = solver(M, 1, 4, 8, tables=[table], obstacles=ob)
    info = np.zeros(6, dtype=M.INFO_DTYPE)
    sampled = s.clearance(sx, sT, 20, 0.0, 0)
    assert np.all(sampled["status"] == 0)
    assert np.array_equal(s.select_clear(sT, info, sampled, group, 2), [0, 4])              # the colliding candidates, "fastest and clean"
    clr, cert = s.clearance_certified(sx, sT, 0.0, 0, 4, 10)
    assert np.array_equal(clr["status"], [1, 0, 0, 0, 1, 0]), clr
    assert np.array_equal(s.select_clear(sT, info, clr, group, 2), [1, 5])
    assert np.array_equal(s.select_checked(sT, info, group, clr=clr, n_groups=2), [1, 5])
    # one level-0 interval per segment and no refinement: nothing can be decided, and no candidate is admitted
    coarse, _ = s.clearance_certified(sx, sT, 0.0, 0, 1, 0)
    assert np.all(coarse["status"] == M.CLR_UNDECIDED), coarse
    assert np.array_equal(s.select_clear(sT, info, coarse, group, 2), [-1, -1])


# ---- 6. routes -----------------------------------------------------------------------------------------------------------------------------------
def test_an_undecided_leg_marks_its_route(M):
    _, _, table, ob, _ = H.thin_capsule_case()
    s = solver(M, 1, 4, 8, tables=[table], obstacles=ob)
    qa, qv, qb = np.array([-0.9, -0.8, 0.2, -2.0, 0.1, 1.8, 0.5]), np.array([0.0, -0.8, 0.2, -1.7, 0.1, 1.8, 0.5]), np.array([1.1, -0.8, 0.2, -1.4, 0.1, 1.8, 0.5])
    legs = np.stack([H.swing(4, qa, qv), H.swing(4, qv, qb)])
    sx = np.ascontiguousarray(np.stack([legs, legs]))                                        # two routes of two legs
    su, sT = np.zeros((2, 2, 13, 7)), np.array([[1.0, 1.0], [1.2, 1.2]])
    info = np.zeros((2, 2), dtype=M.INFO_DTYPE)
    fine, _ = s.clearance_certified(sx.reshape(4, 13, 14), sT.reshape(4), 0.0, 0, 4, 10)
    assert np.all(fine["status"] == 0)
    rT, rinfo, _, rclr = s.route_join(sx, su, sT, info, fine.reshape(2, 2))
    assert np.all(rclr["status"] == 0) and np.array_equal(s.select_clear(rT, rinfo, rclr, np.zeros(2, dtype=np.int32), 1), [0])
    # the first leg of route 0 checked without refinement is undecided: the bit reaches the route record and route 1 is chosen
    coarse, _ = s.clearance_certified(sx[0, 0:1], sT[0, 0:1], 0.0, 0, 1, 0)
    assert coarse["status"][0] == M.CLR_UNDECIDED
    mixed = fine.reshape(2, 2).copy(); mixed[0, 0] = coarse[0]
    rT, rinfo, _, rclr = s.route_join(sx, su, sT, info, mixed)
    assert rclr["status"][0] == M.CLR_UNDECIDED and rclr["status"][1] == 0
    assert np.array_equal(s.select_clear(rT, rinfo, rclr, np.zeros(2, dtype=np.int32), 1), [1])
    mixed[1, 0] = coarse[0]
    rclr = s.route_join(sx, su, sT, info, mixed)[3]
    assert np.array_equal(s.select_clear(rT, rinfo, rclr, np.zeros(2, dtype=np.int32), 1), [-1])


# ---- 7. NaN nodes ----------------------------------------------------------------------------------------------------------------------------------
def test_a_stopped_tool_line_is_reported_as_nan(M):
    s = solver(M, 1, 4, 4, obstacles=H.world(1))
    q = np.array([[0.3, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5]] * 2)
    _, p0, R0 = M.tool_jacobian(H.robot(1)[0][0], q[0])
    p1 = np.stack([p0 + [0.0, 0.0, 0.1], p0 + p0 / np.linalg.norm(p0) * 3.0])               # a lift, and a line straight out of the workspace
    sx, _, sT, rec = s.tool_line(q, np.stack([R0, R0]), p1)
    assert rec["status"][0] == 0 and rec["status"][1] & M.TL_STOPPED and np.isnan(sx[1]).any()
    clr, cert = s.clearance_certified(sx, sT, MARGIN, 0, 4, 10)
    assert clr["status"][1] == M.CLR_NAN and np.isnan(clr["d_min"][1]) and clr["t_min"][1] == -1.0 and clr["n_hit"][1] == 0 and clr["sphere"][1] == -1
    assert np.isnan(cert["d_lower"][1]) and cert["t_lower"][1] == -1.0 and cert["n_eval"][1] == 0 and cert["depth"][1] == 0
    assert clr["status"][0] != M.CLR_NAN and np.isfinite(cert["d_lower"][0]) and cert["n_eval"][0] >= 16


# ---- 8. the device variant on a caller's stream ---------------------------------------------------------------------------------------------
def test_device_variant_on_a_stream(M):
    import torch
    x, T = H.plans(1, 4, 15)
    B = x.shape[0]
    s = solver(M, 1, 4, B, obstacles=H.world(1))
    clr, cert = s.clearance_certified(x, T, MARGIN, 4, 4, 10)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dx, dT = torch.from_numpy(x).cuda(), torch.from_numpy(T).cuda()
        dclr = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dcert = torch.zeros(B * M.CLEARANCE_CERT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        s.clearance_certified_device(B, dx.data_ptr(), dT.data_ptr(), MARGIN, 4, 4, 10, dclr.data_ptr(), dcert.data_ptr(), stream=st.cuda_stream)
        dsel = torch.zeros(1, dtype=torch.int32, device="cuda")
        dinfo = torch.zeros(B * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dgrp = torch.zeros(B, dtype=torch.int32, device="cuda")
        s.select_clear_device(B, dT.data_ptr(), dinfo.data_ptr(), dclr.data_ptr(), dgrp.data_ptr(), 1, dsel.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert dclr.cpu().numpy().tobytes() == clr.tobytes() and dcert.cpu().numpy().tobytes() == cert.tobytes()
    ok = np.flatnonzero(clr["status"] == 0)
    assert ok.size and int(dsel.cpu()[0]) == ok[np.lexsort((ok, T[ok]))[0]]
    # refused calls write nothing
    L, ctx = M.lib(), s._ctx
    before = dclr.clone()
    for kw in (dict(B=0), dict(n_start=0), dict(n_start=1025), dict(max_depth=17), dict(max_depth=-1), dict(margin=float("nan")), dict(gap=-1),
               dict(x=None), dict(T=None), dict(out=None)):
        a = dict(B=B, x=dx.data_ptr(), T=dT.data_ptr(), margin=MARGIN, gap=0, n_start=4, max_depth=10, out=dclr.data_ptr())
        a.update(kw)
        assert L.mpcmp_clearance_certified_batch_device(ctx, a["B"], a["x"], a["T"], a["margin"], a["gap"], a["n_start"], a["max_depth"], a["out"],
                                                        dcert.data_ptr(), None) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(before, dclr)
    host_out = np.zeros(B, dtype=M.CLEARANCE_DTYPE); host_out["n_hit"] = 77
    assert L.mpcmp_clearance_certified_batch(ctx, B, x.ctypes.data, T.ctypes.data, MARGIN, 0, 4, 17, host_out.ctypes.data, None) == -1
    assert L.mpcmp_clearance_certified_batch(None, B, x.ctypes.data, T.ctypes.data, MARGIN, 0, 4, 10, host_out.ctypes.data, None) == -1
    assert np.all(host_out["n_hit"] == 77)


# ---- 9. the façade ---------------------------------------------------------------------------------------------------------------------------------
def test_planner_facade(M):
    from mpc_motion_planner_amd import scenarios
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    p.set_constraint_margins(*MARGINS)
    x0, xf = scenarios.make_batch(8, MARGINS)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    p.set_obstacles(H.world(1))
    clr, cert = p.check_clearance_certified(margin=MARGIN, n_start=4, max_depth=8)
    sx, _, sT = p.solution()
    s = solver(M, 1, 4, 8, tables=[M.link_spheres(p.model, 0.06, 0.08)], obstacles=H.world(1))      # (the façade's robot: the whole skeleton)
    c2, t2 = s.clearance_certified(sx, sT, MARGIN, 0, 4, 8)
    assert clr.tobytes() == c2.tobytes() and cert.tobytes() == t2.tobytes() and clr.dtype == M.CLEARANCE_DTYPE and cert.dtype == M.CLEARANCE_CERT_DTYPE
    sampled = p.check_clearance(n_pts=200, margin=MARGIN)
    for b in range(8):                      # a certified plan has no sample below the margin; the samples cannot lie below the bound
        assert sampled["d_min"][b] >= cert["d_lower"][b] - 1e-12
        assert clr["status"][b] != 0 or sampled["status"][b] == 0


# ---- 10. the C++ shim --------------------------------------------------------------------------------------------------------------------------------
def test_cpp_shim_member(M, tmp_path):
    """examples/clearance_cert_selftest.cpp builds with plain g++ -Wall -Werror against the library and prints consistent records"""
    exe = str(tmp_path / "clearance_cert_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "clearance_cert_selftest.cpp"), "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    host, shim = [json.loads(l) for l in r.stdout.strip().split("\n")]
    assert len(host["host"]) == 6
    assert shim["tl_status"] == 0 and shim["sampled_status"] == 0 and shim["status"] == 0 and shim["coarse_status"] in (0, 4)
    assert shim["d_lower"] <= shim["d_min"] <= shim["sampled_d_min"] + 1e-4 and shim["d_lower"] >= 0.02
    assert shim["n_eval"] >= 32 and shim["n_undecided"] == 0 and shim["n_clear"] >= 32 and 0 <= shim["depth"] <= 10
