"""Certified clearance in a moving world on the GPU (mpcmp_clearance_certified_timed_batch*, include/mpcmp_moving_cert.h): the kernel against the
host statement of the rule and against the NumPy reference on the cases of tests/test_moving_cert_host.py (where the reference's decision gaps and
the spread of hits and certificates are asserted), independence of the batch, the static certificate as a special case, what samples cannot see and
its way through the selection, the capacity rule, the device variant, the certified start search, the façade and the C++ shim.

Shapes.  B = 12 and num_seg <= 6, the host cases: one arm at num_seg 1 (all intervals share their cubic), two arms at num_seg 6, 1 and 64 tracks,
chunks that mix rest and motion intervals (n_rest 3 with n_start 1), and the capacity case with more than 2,048 splits of a level.

Bounds.  Integers equal, doubles within 1e-12 (1 + |x|), as between the host statement and the reference: kernel and host statement run one source,
the kernel with contracted multiply-adds and the device's sine and cosine.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import clearance_cert_reference as R
import moving_cert_reference as MC
import test_clearance_cert_host as H
import test_moving_cert_host as MH

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def solver(M, narm, nseg, max_batch, tables=None, obstacles=None, tracks=None):
    """tracks: (track_of, offsets, t0, dt), for one world or stacked per problem"""
    models, _, tabs = H.robot(narm)
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    for a, t in enumerate(tabs if tables is None else tables):
        s.set_robot_spheres(t, arm=a)
    if obstacles is not None:
        s.set_obstacles(obstacles)
    if tracks is not None:
        s.set_obstacle_tracks(*tracks)
    return s


def world_of(d, idx, per_problem):
    """the obstacle sets and track table of the problems idx of a case's data, as Solver takes them"""
    if not per_problem:
        return d["obs"][0], d["tracks"][0]
    tr = [d["tracks"][b] for b in idx]
    return (np.ascontiguousarray(np.stack([d["obs"][b] for b in idx])),
            (np.stack([t[0] for t in tr]), np.ascontiguousarray(np.stack([t[1] for t in tr])), tr[0][2], tr[0][3]))


def run_case(s, case, d, idx):
    idx = np.asarray(idx)
    return s.clearance_certified_timed(np.ascontiguousarray(d["x"][idx]), d["T"][idx], d["ts"][idx], d["w"][idx], d["h"][idx], case.margin,
                                       case.self_gap, case.n_start, case.n_rest, case.max_depth)


# ---- 1., 2. the kernel against the host statement and the reference; cert may be left out ----------------------------------------------------
@pytest.mark.parametrize("case", MH.CASES, ids=MH.IDS)
def test_kernel_matches_host_statement_and_reference(M, case):
    ref = MH.case_reference(case)
    MH.assert_fair(case, ref)
    d = MH.case_data(case)
    idx = np.arange(MH.NP)
    obs, tracks = world_of(d, idx, case.per_problem)
    s = solver(M, case.narm, case.nseg, MH.NP, obstacles=obs, tracks=tracks)
    clr, cert = run_case(s, case, d, idx)
    for b in range(MH.NP):
        hc, ht = MH.one_of_case(M, case, b)
        H.check_records(clr[b], cert[b], dict(clr=hc, cert=ht), ("host", case.name, b))
        H.check_records(clr[b], cert[b], ref[b], ("reference", case.name, b))
    only = np.zeros(MH.NP, dtype=M.CLEARANCE_DTYPE)
    x, T, ts, w, h = (np.ascontiguousarray(d[k]) for k in ("x", "T", "ts", "w", "h"))
    assert M.lib().mpcmp_clearance_certified_timed_batch(s._ctx, MH.NP, x.ctypes.data, T.ctypes.data, ts.ctypes.data, w.ctypes.data, h.ctypes.data,
                                                         case.margin, case.self_gap, case.n_start, case.n_rest, case.max_depth, only.ctypes.data,
                                                         None) == 0
    assert only.tobytes() == clr.tobytes()


# ---- 3. a plan's records do not depend on the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [MH.CASES[2], MH.CASES[3]], ids=[MH.IDS[2], MH.IDS[3]])
def test_records_do_not_depend_on_the_batch(M, case):
    """alone, in a batch of 33 and reversed, bitwise: one world with 64 tracks, and one obstacle set and track table per problem"""
    d = MH.case_data(case)
    idx = np.arange(33) % MH.NP
    obs, tracks = world_of(d, idx, case.per_problem)
    s = solver(M, case.narm, case.nseg, 33, obstacles=obs, tracks=tracks)
    clr, cert = run_case(s, case, d, idx)
    rev = idx[::-1]
    if case.per_problem:
        obs_r, tracks_r = world_of(d, rev, True)
        s.set_obstacles(obs_r); s.set_obstacle_tracks(*tracks_r)
    clr_r, cert_r = run_case(s, case, d, rev)
    assert clr_r[::-1].tobytes() == clr.tobytes() and cert_r[::-1].tobytes() == cert.tobytes()
    for b in (0, 7, 20, 32):
        if case.per_problem:
            obs_1, tracks_1 = world_of(d, idx[b:b + 1], True)
            s.set_obstacles(obs_1); s.set_obstacle_tracks(*tracks_1)
        c1, t1 = run_case(s, case, d, idx[b:b + 1])
        assert c1.tobytes() == clr[b:b + 1].tobytes() and t1.tobytes() == cert[b:b + 1].tobytes(), b
    assert len(set(clr["status"].tolist())) >= 2


# ---- 4. no tracks and no rests: the static certificate ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm,nseg,self_gap,n_start,max_depth,seed", [H.CASES[1], H.CASES[4], H.CASES[6]])
def test_static_world_without_rests_is_the_static_certificate(M, narm, nseg, self_gap, n_start, max_depth, seed):
    x, T = H.plans(narm, nseg, seed)
    s = solver(M, narm, nseg, x.shape[0], obstacles=H.world(narm))
    clr0, cert0 = s.clearance_certified(x, T, H.MARGIN, self_gap, n_start, max_depth)
    for ts in (None, -3.25, 17.0):
        clr, cert = s.clearance_certified_timed(x, T, ts, None, 0.0, H.MARGIN, self_gap, n_start, 2, max_depth)
        for b in range(x.shape[0]):
            H.check_records(clr[b], cert[b], dict(clr=clr0[b], cert=cert0[b]), ("static", narm, nseg, b, ts))


# ---- 5. what samples cannot see, followed through the selection ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_selection_takes_the_certified_candidate(M, which):
    """a crossing between samples of the motion (a), an arrival during the hold (b), a crossing of the waiting robot (c): from the timed records the
    selection picks the faster candidate, which collides; from the certified records the clean one.  n_rest = 3: with an even count the obstacle of
    (b) would pass the resting sphere exactly on an interval boundary, and the two leaves beside it would tie in d_lower up to the last bit"""
    x, T, table, obs, tracks, ts, w, h = MH.selection_case(which)
    s = solver(M, 1, 4, 4, tables=[table], obstacles=obs, tracks=tracks)
    info, group = np.zeros(2, dtype=M.INFO_DTYPE), np.zeros(2, dtype=np.int32)
    timed = s.clearance_timed(x, T, None, ts, 20, 0.0)
    assert np.all(timed["status"] == 0), timed
    assert np.array_equal(s.select_clear(T, info, timed, group, 1), [0])
    clr, cert = s.clearance_certified_timed(x, T, ts, w, h, 0.0, 0, 4, 3, 10)
    assert clr["status"][0] & M.CLR_HIT and clr["status"][1] == 0 and clr["d_min"][0] < 0.0, (clr, cert)
    when = {"a": 0.74, "b": T[0] + 0.05, "c": 0.25}[which]
    assert abs(clr["t_min"][0] - when) < 0.005, (which, clr["t_min"][0])
    assert np.array_equal(s.select_clear(T, info, clr, group, 1), [1])
    assert np.array_equal(s.select_checked(T, info, group, clr=clr, n_groups=1), [1])
    for b in range(2):
        hc, ht = MH.one(M, 1, 4, obs, tracks, x[b], T[b], ts, w, h, 0.0, 0, 4, 3, 10, tables=[table])
        H.check_records(clr[b], cert[b], dict(clr=hc, cert=ht), (which, b))
    if which == "b":                    # the plan alone, without its hold, is certified clear
        assert s.clearance_certified_timed(x, T, ts, 0.0, 0.0, 0.0, 0, 4, 3, 10)[0]["status"][0] == 0


# ---- 6. capacity and depth --------------------------------------------------------------------------------------------------------------------
def test_capacity_with_rest_intervals_and_a_deep_hit(M):
    """n0 = 4096 with 2 x 8 rest intervals and the long graze of the host test (2,048 splits of level 0, 8,192 evaluations), and max_depth 16 on a
    hit deep in the tree: against the host statement, whose agreement with the reference the host test asserts"""
    _, arrays, _ = H.robot(1)
    nseg, n_start, n_rest = 4, 1020, 8
    q0 = np.array([-1.0, -0.5, 0.0, -2.0, 0.0, 1.6, 0.0]); q1 = q0.copy(); q1[0] = 1.0; q1[1] = -0.5 + 1e-5
    tau = M.time_nodes(nseg)
    x = np.zeros((1, tau.shape[0], 14)); x[0, :, :7] = q0[None] + (q1 - q0)[None] * tau[:, None]
    table = M.spheres([3], [[0.0, 0.0, 0.0]], 0.05)
    z = [R.frames(arrays[0], R.position(nseg, x[0], t))[1][3][2] for t in np.linspace(0.0, 1.0, 2001)]
    ob = np.array([M.obstacle(M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (min(z) - 0.05 - H.MARGIN - 1e-5, 0, 0), 0.0)], dtype=M.OBSTACLE_DTYPE)
    s = solver(M, 1, nseg, 2, tables=[table], obstacles=ob)
    clr, cert = s.clearance_certified_timed(x, np.array([2.0]), 0.5, 0.25, 0.75, H.MARGIN, 0, n_start, n_rest, 1)
    hc, ht = MH.one(M, 1, nseg, ob, None, x[0], 2.0, 0.5, 0.25, 0.75, H.MARGIN, 0, n_start, n_rest, 1, tables=[table])
    H.check_records(clr[0], cert[0], dict(clr=hc, cert=ht), "capacity")
    assert cert["n_eval"][0] == 8192 and clr["status"][0] == M.CLR_UNDECIDED and cert["n_undecided"][0] >= 2048 + 4096 - 16
    cc = MH.crossing_case(0.37, 0.3 + 0.74, lateral=0.008 - 5e-6)
    s2 = solver(M, 1, 4, 2, tables=[cc.table], obstacles=cc.obs, tracks=cc.tracks)
    clr, cert = s2.clearance_certified_timed(cc.x[None], np.array([cc.T]), 0.3, 0.1, 0.1, 0.0, 0, 1, 1, 16)
    hc, ht = MH.one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, 0.3, 0.1, 0.1, 0.0, 0, 1, 1, 16, tables=[cc.table])
    H.check_records(clr[0], cert[0], dict(clr=hc, cert=ht), "deep hit")
    assert clr["status"][0] & M.CLR_HIT and cert["depth"][0] >= 10


# ---- 7. the device variant on a caller's stream ---------------------------------------------------------------------------------------------
def test_device_variant_on_a_stream(M):
    import torch
    case = MH.CASES[3]
    d = MH.case_data(case)
    B = MH.NP
    obs, tracks = world_of(d, np.arange(B), True)
    s = solver(M, case.narm, case.nseg, B, obstacles=obs, tracks=tracks)
    clr, cert = run_case(s, case, d, np.arange(B))
    st = torch.cuda.Stream()

    def call(dx, dT, dts, dw, dh, dclr, dcert):
        s.clearance_certified_timed_device(B, dx.data_ptr(), dT.data_ptr(), dts.data_ptr(), dw.data_ptr(), dh.data_ptr(), case.margin, case.self_gap,
                                           case.n_start, case.n_rest, case.max_depth, dclr.data_ptr(), dcert.data_ptr(), stream=st.cuda_stream)
    with torch.cuda.stream(st):
        dx, dT, dts, dw, dh = (torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("x", "T", "ts", "w", "h"))
        dclr = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dcert = torch.zeros(B * M.CLEARANCE_CERT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dclr2, dcert2 = torch.zeros_like(dclr), torch.zeros_like(dcert)
        call(dx, dT, dts, dw, dh, dclr, dcert)
    st.synchronize()
    assert dclr.cpu().numpy().tobytes() == clr.tobytes() and dcert.cpu().numpy().tobytes() == cert.tobytes()
    # a second call on the same context allocates nothing: the device's free memory is what it was (the outputs exist already)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    with torch.cuda.stream(st):
        call(dx, dT, dts, dw, dh, dclr2, dcert2)
    st.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before
    assert torch.equal(dclr, dclr2) and torch.equal(dcert, dcert2)
    # a negative duration is not looked at by the device call: the NaN record; the host-pointer call refuses it and writes nothing
    with torch.cuda.stream(st):
        dneg = dw.clone(); dneg[3] = -0.25
        call(dx, dT, dts, dneg, dh, dclr2, dcert2)
    st.synchronize()
    got = np.frombuffer(dclr2.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)
    gcert = np.frombuffer(dcert2.cpu().numpy().tobytes(), dtype=M.CLEARANCE_CERT_DTYPE)
    assert got["status"][3] == M.CLR_NAN and np.isnan(got["d_min"][3]) and got["t_min"][3] == -1.0 and np.isnan(gcert["d_lower"][3]) and gcert["n_eval"][3] == 0
    keep = np.arange(B) != 3
    assert got[keep].tobytes() == clr[keep].tobytes() and gcert[keep].tobytes() == cert[keep].tobytes()
    L, ctx = M.lib(), s._ctx
    x, T, ts, w, h = (np.ascontiguousarray(d[k]) for k in ("x", "T", "ts", "w", "h"))
    host_out = np.zeros(B, dtype=M.CLEARANCE_DTYPE); host_out["n_hit"] = 77
    wneg = w.copy(); wneg[3] = -0.25
    hneg = h.copy(); hneg[11] = -1e-9
    for kw in (dict(w=wneg), dict(h=hneg), dict(n_rest=0), dict(n_start=1023, n_rest=3), dict(max_depth=17), dict(B=0), dict(margin=float("nan")), dict(x=None)):
        a = dict(B=B, x=x.ctypes.data, w=w, h=h, margin=case.margin, n_start=4, n_rest=3, max_depth=10)
        a.update(kw)
        assert L.mpcmp_clearance_certified_timed_batch(ctx, a["B"], a["x"], T.ctypes.data, ts.ctypes.data, a["w"].ctypes.data, a["h"].ctypes.data,
                                                       a["margin"], 0, a["n_start"], a["n_rest"], a["max_depth"], host_out.ctypes.data, None) == -1, kw
    before = dclr.clone()
    for kw in (dict(n_rest=0), dict(n_start=1023, n_rest=3), dict(max_depth=-1), dict(out=None)):
        a = dict(n_start=4, n_rest=3, max_depth=10, out=dclr.data_ptr())
        a.update(kw)
        assert L.mpcmp_clearance_certified_timed_batch_device(ctx, B, dx.data_ptr(), dT.data_ptr(), dts.data_ptr(), dw.data_ptr(), dh.data_ptr(), case.margin,
                                                              0, a["n_start"], a["n_rest"], a["max_depth"], a["out"], dcert.data_ptr(), None) == -1, kw
    torch.cuda.synchronize()
    assert np.all(host_out["n_hit"] == 77) and torch.equal(before, dclr)


# ---- 8. the certified start search -------------------------------------------------------------------------------------------------------------
def planner_with_plans(M, x, T, table, obs, tracks):
    """a BatchMotionPlanner whose last solution is the given plans (the search reads nothing else of a solve)"""
    p = M.BatchMotionPlanner(max_batch=x.shape[0], num_seg=4, sqp_iters=1)
    p._sol, p._route = (np.ascontiguousarray(x), np.zeros((x.shape[0], x.shape[1], 7)), np.ascontiguousarray(T)), None
    p.set_obstacles(obs, spheres=table)
    p.set_moving_obstacles(*tracks)
    return p


def test_first_certified_start(M):
    """case (c) in a batch of 4 (tests/test_moving_cert_host.search_batch).  Problem 1: the sampled search calls the delay 0 clear, its certified record
    is a hit between samples, and the search returns the next delay with status 0.  Problem 0, case (c) itself: the run that starts at once is
    certified (the robot has left when the obstacle comes); every later delay has the crossing in its wait, a wait only grows with the delay, so the
    search can never return the delay 0.5 that the sampled wait check calls clear"""
    x, T, table, obs, tracks = MH.search_batch()
    want, _, sampled = MH.certified_start_on_the_host(M, x, T, table, obs, tracks, MH.C_DELAYS)
    p = planner_with_plans(M, x, T, table, obs, tracks)
    rec, _ = p.first_clear_start(MH.C_DELAYS, True, 20, 0.0)
    assert rec["index"].tolist() == sampled == [0, 0, 0, 0]
    index, clr, cert = p.first_certified_start(MH.C_DELAYS, margin=0.0, n_pts=20)
    assert index.tolist() == want == [0, 1, 0, 0], (index, want)
    assert np.all(clr["status"] == 0) and np.all(cert["d_lower"] >= 0.0)
    first = p.check_clearance_certified_timed(MH.C_DELAYS[0], 0.0, None)[0]
    assert first["status"][1] & M.CLR_HIT and abs(first["t_min"][1] - 0.74) < 0.005
    # one round only: problem 1 finds no certified delay, and its record is the hit
    index, clr, _ = p.first_certified_start(MH.C_DELAYS, margin=0.0, n_pts=20, max_rounds=1)
    assert index.tolist() == [0, -1, 0, 0] and clr["status"][1] & M.CLR_HIT
    # the waiting robot of case (c): started at 0.5 or 1.0 it is hit during its wait
    later = p.check_clearance_certified_timed(MH.C_DELAYS[1], MH.C_DELAYS[1] - MH.C_DELAYS[0], None)[0]
    assert later["status"][0] & M.CLR_HIT and abs(later["t_min"][0] - 0.25) < 0.005
    with pytest.raises(ValueError):
        p.check_clearance_certified_timed(retimed=True)


# ---- 9. the façade and the shim ----------------------------------------------------------------------------------------------------------------
def test_planner_facade(M):
    from mpc_motion_planner_amd import scenarios
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    p.set_constraint_margins(*MARGINS)
    x0, xf = scenarios.make_batch(8, MARGINS)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    d = MH.case_data(MH.CASES[2])
    obs, tracks = d["obs"][0], d["tracks"][0]
    p.set_obstacles(obs)
    p.set_moving_obstacles(*tracks)
    ts, w, h = 0.7 + 0.05 * np.arange(8), 0.3, np.linspace(0.0, 0.7, 8)
    clr, cert = p.check_clearance_certified_timed(ts, w, h, margin=H.MARGIN, n_start=4, n_rest=3, max_depth=8)
    sx, _, sT = p.solution()
    s = solver(M, 1, 4, 8, tables=[M.link_spheres(p.model, 0.06, 0.08)], obstacles=obs, tracks=tracks)      # (the façade's robot: the whole skeleton)
    c2, t2 = s.clearance_certified_timed(sx, sT, ts, w, h, H.MARGIN, 0, 4, 3, 8)
    assert clr.tobytes() == c2.tobytes() and cert.tobytes() == t2.tobytes() and clr.dtype == M.CLEARANCE_DTYPE and cert.dtype == M.CLEARANCE_CERT_DTYPE
    sampled = p.check_clearance_timed(ts, 200, H.MARGIN)
    for b in range(8):                      # a certified plan has no sample below the margin; the samples cannot lie below the bound
        assert sampled["d_min"][b] >= cert["d_lower"][b] - 1e-12
        assert clr["status"][b] != 0 or sampled["status"][b] == 0
    hc, ht = M.clearance_certified_timed_one([p.model], 4, [M.link_spheres(p.model, 0.06, 0.08)], obs, tracks, sx[2], sT[2], ts[2], w, h[2], H.MARGIN, 0, 4, 3, 8)
    H.check_records(clr[2], cert[2], dict(clr=hc, cert=ht), "facade against host")
    with pytest.raises(ValueError):
        p.check_clearance_certified_timed(retimed=True)


def test_cpp_shim_member(M, tmp_path):
    """examples/moving_cert_selftest.cpp builds with plain g++ -Wall -Werror against the library and prints consistent records"""
    exe = str(tmp_path / "moving_cert_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "moving_cert_selftest.cpp"), "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    host, shim = [json.loads(l) for l in r.stdout.strip().split("\n")]
    assert len(host["host"]) == 2
    # the world at rest: the static certificate's record; the pole: a hit between the bounds; the late start behind the pole: consistent bounds
    assert shim["still_status"] == shim["static_status"] and shim["still_n_eval"] == shim["static_n_eval"]
    assert abs(shim["still_d_min"] - shim["static_d_min"]) <= 1e-12 and abs(shim["still_d_lower"] - shim["static_d_lower"]) <= 1e-12
    for k in ("still", "meet", "late"):          # (the solved move is the solver's: only what holds for any plan is asserted of the moving world)
        assert shim[k + "_d_lower"] <= shim[k + "_d_min"] and bool(shim[k + "_status"] & 1) == (shim[k + "_d_min"] < 0.02), (k, shim)
        assert shim[k + "_status"] != 0 or shim[k + "_d_lower"] >= 0.02, (k, shim)
    assert 0.0 <= shim["late_t_min"] <= 4.0 + 10.0 + 1.0
