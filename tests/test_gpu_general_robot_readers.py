"""The readers of a finished plan on the GPU, on robots that are NOT the Panda.  Run with -m gpu.

tests/test_gpu_general_robot.py took the rigid-body leaf kernels, k_clearance, the pose targets and the QP paths off the Panda.  The kernels that
read a finished plan came later, each with its own chain code or its own way of indexing the per-arm and per-problem model array, and saw only
Panda constants: k_limits, k_retime, k_sample_retimed, k_limits_retimed, k_sample_route, k_clearance_cert without and with a timeline, and the kernels
of moving.hip.  Here they run on general_11, tilted_14 (gravity with three components), dual_21 (two DIFFERENT chains) and general_12 /
dual_21 under per-problem payload rows, on the cases tests/test_general_robot_readers_host.py chooses and qualifies on the CPU (its docstring states
the shapes, the bounds and the fairness conditions, which are asserted here again on the same cached references), against the same references and
with the same check functions as the Panda modules.  A kernel that stages arm 0's placements for arm 1, indexes b * mstride + a wrongly, drops a
component of p or an off-diagonal of R0, or splits the torque for gravity along z only fails here and nowhere else.

mpcmp_sample_route_batch is a one-arm entry point (it refuses a two-arm context), so it runs on general_11 only.
"""
import numpy as np
import pytest

import moving_reference as mr
import retime_reference as RT
import route_retime_reference as RR
import test_clearance_cert_host as H
import test_general_robot_readers_host as G
import test_gpu_limits as GL
import test_limits_host as LH
import test_moving_cert_host as MH
import test_moving_world_host as MW
import test_retime_host as TH
import test_retimed_check_host as CH
import test_route_retime_host as RH

pytestmark = pytest.mark.gpu
B, N_PTS, N_GRID, NVIA, TOL = G.B, G.N_PTS, G.N_GRID, G.NVIA, G.TOL


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def solver(M, name, max_batch=B, models=None):
    narm, nseg = G.shape(name)
    return GL.solver(M, narm, nseg, max_batch, models=G.models(name) if models is None else models)


def set_payloads(s, name, swap=False):
    mass, com, inertia = G.payload_table(name)
    if swap:
        mass, com, inertia = mass[:, ::-1], com[:, ::-1], inertia[:, ::-1]
    if mass.shape[1] == 1:
        mass, com, inertia = mass[:, 0], com[:, 0], inertia[:, 0]
    s.set_payloads(np.ascontiguousarray(mass), np.ascontiguousarray(com), np.ascontiguousarray(inertia))


# ---- 1. limits, retime, sample_retimed, limits_retimed: plain rows and payload rows (one arm and two: b * mstride + a) -------------------------
@pytest.mark.parametrize("name,payload", G.CASES_23, ids=G.IDS_23)
def test_limits_retime_and_retimed_limits_vs_reference(M, name, payload):
    c = G.reader_case(name, payload)
    G.assert_limits_case_is_fair(c["lim_ref"], name)
    G.assert_retime_case_is_fair(c["rt_ref"], c["amp"], name)
    per = lambda b: c["models"][b] if payload else c["models"]
    sx, su, sT, lin_max, ang_max = c["sx"], c["su"], c["sT"], c["lin_max"], c["ang_max"]
    s = solver(M, name)
    s.set_bounds(c["table"])
    if payload:
        set_payloads(s, name)
    worst = np.zeros(LH.GROUPS)
    GL.check_records(s.limits(sx, su, sT, N_PTS, TOL, lin_max, ang_max), c["lim_ref"], sT, N_PTS, TOL, (name, "limits"), worst)
    prof, rec = s.retime(sx, su, sT, N_GRID, M.retime_spec(lin_max, ang_max))
    dev = [0.0, 0.0]
    TH.check_against(c["rt_ref"], prof, rec, what=(name, "retime"), worst=dev)
    for b in np.flatnonzero(rec["status"] == 0):
        TH.check_limits_hold(dict(P=c["P"][b], T=sT[b]), c["table"][b], prof[b, :, 1], lin_max, ang_max, what=(name, b))
    # the sampler under the GPU's own profiles: the torque column is that of the (lumped) model of the problem
    got = s.sample_retimed(sx, su, sT, prof, N_PTS)
    sdev = 0.0
    for b in range(B):
        if rec[b]["status"]:
            assert np.isnan(got[b]).all(), (name, b)
            continue
        want = RT.sample_retimed_np(per(b), c["nseg"], sx[b], su[b], sT[b], prof[b], N_PTS)
        sdev = max(sdev, np.abs(got[b] - want).max())
        assert np.abs(got[b] - want).max() <= 1e-9, (name, b, np.abs(got[b] - want).max())
    # the retimed plans between the grid points, under the check rows
    table = G.check_rows(M, name)
    s.set_bounds(table)
    ref = CH.plan_references(c["models"], c["nseg"], sx, su, sT, prof, table, N_PTS, lin_max, ang_max)
    G.assert_retimed_case_is_fair(ref, name)
    lim, T_new = s.limits_retimed(sx, su, sT, prof, N_PTS, TOL, lin_max, ang_max)
    assert [r["failed"] for r in ref] == list(rec["status"] != 0)
    worst2 = np.zeros(LH.GROUPS)
    CH.check_retimed(M, lim, T_new, ref, N_PTS, what=(name, "limits_retimed"), worst=worst2)
    print("%s%s: max |excess - ref| per group %s; retime |x / ref - 1| %.1e, |T_new / ref - 1| %.1e; sampler %.1e; retimed excess %s"
          % (name, " payloads" if payload else "", " ".join("%.1e" % w for w in worst), dev[0], dev[1], sdev, " ".join("%.1e" % w for w in worst2)))
    if payload:          # the rows are felt: cleared, the torque group moves
        s.clear_payloads()
        bare, _ = s.limits_retimed(sx, su, sT, prof, N_PTS, TOL, lin_max, ang_max)
        ok = rec["status"] == 0
        assert (np.abs(bare["excess"][ok, LH.TAU] - lim["excess"][ok, LH.TAU]) > 1e-3).any()


# ---- 2. routes of two legs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.MOVING)
def test_route_readers_vs_reference(M, name):
    c = G.route_case(name)
    G.assert_route_case_is_fair(c["ref"], c["amp"], name)
    sx, su, sT, lin_max, ang_max = c["sx"], c["su"], c["sT"], c["lin_max"], c["ang_max"]
    s = solver(M, name, B * (NVIA + 1))
    s.set_bounds(np.ascontiguousarray(c["table"]).reshape(-1))
    prof, leg_T, rec = s.retime_route(sx, su, sT, N_GRID, M.retime_spec(lin_max, ang_max))
    assert RH.check_route_against(c["ref"], prof, leg_T, rec, what=name) == 0
    got = s.sample_retimed_route(sx, su, sT, prof, N_PTS)
    ident = np.ones((B, NVIA + 1, N_GRID + 1, 2))
    ident[..., 0] = (np.arange(N_GRID + 1) / N_GRID)[None, None, :] * sT[:, :, None]
    plain = s.sample_route(sx, su, sT, N_PTS) if c["narm"] == 1 else None
    for b in range(B):
        if rec[b]["status"]:
            assert np.isnan(got[b]).all(), (name, b)
        else:
            want = RR.sample_retimed_route_np(c["models"], c["nseg"], sx[b], su[b], sT[b], prof[b], N_PTS)
            assert np.abs(got[b] - want).max() <= 1e-9, (name, b, np.abs(got[b] - want).max())
        if plain is not None:          # the route sampler is the retimed one under a profile of ones: the torque column of every leg
            want = RR.sample_retimed_route_np(c["models"], c["nseg"], sx[b], su[b], sT[b], ident[b], N_PTS)
            assert np.abs(plain[b] - want).max() <= 1e-9, (name, b, np.abs(plain[b] - want).max())
    # the retimed routes between the grid points, under the check rows: every group has a route over and a clean one
    s.set_bounds(np.ascontiguousarray(c["check"]).reshape(-1))
    ref = CH.route_references(c["models"], c["nseg"], sx, su, sT, prof, c["check"], N_PTS, lin_max, ang_max)
    G.assert_retimed_case_is_fair(ref, name)
    lim, T_new = s.limits_retimed_route(sx, su, sT, prof, N_PTS, TOL, lin_max, ang_max)
    CH.check_retimed(M, lim, T_new, ref, N_PTS, what=(name, "routes"))


# ---- 3. the certificate -----------------------------------------------------------------------------------------------------------------------
def cert_solver(M, name, max_batch, obstacles=None, tracks=None, models=None, tables=None):
    s = solver(M, name, max_batch, models)
    for a, t in enumerate(G.cert_tables(name) if tables is None else tables):
        s.set_robot_spheres(t, arm=a)
    if obstacles is not None:
        s.set_obstacles(obstacles)
    if tracks is not None:
        s.set_obstacle_tracks(*tracks)
    return s


@pytest.mark.parametrize("name,seed,depth", [(n, None, None) for n in G.READERS] + [G.DEEP], ids=list(G.READERS) + ["deep"])
def test_certified_vs_host_statement_and_reference(M, name, seed, depth):
    """self_gap on for the one-arm robots (3), per-arm tables that differ on dual_21; and the plans that split down to level 10"""
    ref = G.cert_reference(name, seed, depth)
    if depth is None:
        G.assert_cert_case_is_fair(ref, name)
    else:
        assert min(r["gap"] for r in ref) > H.GAP and sum(r["cert"]["depth"] == depth for r in ref) >= 2
    narm, nseg = G.shape(name)
    self_gap, _, n_start, d0, _ = G.CERT_CASES[name]
    depth = d0 if depth is None else depth
    ms, _, tables = G.cert_robot(name)
    x, T = G.cert_plans(name, seed)
    s = cert_solver(M, name, B, G.cert_world(name))
    clr, cert = s.clearance_certified(x, T, G.MARGIN, self_gap, n_start, depth)
    for b in range(B):
        hc, ht = H.one(M, narm, nseg, G.cert_world(name), x[b], T[b], G.MARGIN, self_gap, n_start, depth, tables=tables, models=ms)
        H.check_records(clr[b], cert[b], dict(clr=hc, cert=ht), ("host", name, b))
        H.check_records(clr[b], cert[b], ref[b], ("reference", name, b))


def test_a_certified_record_does_not_depend_on_the_batch(M):
    """dual_21: the records of a batch of 33, and four of its plans alone, bitwise"""
    name = "dual_21"
    self_gap, _, n_start, depth, _ = G.CERT_CASES[name]
    x8, T8 = G.cert_plans(name)
    idx = np.arange(33) % B
    x, T = np.ascontiguousarray(x8[idx]), np.ascontiguousarray(T8[idx] * (1.0 + 0.01 * np.arange(33)))
    s = cert_solver(M, name, 33, G.cert_world(name))
    clr, cert = s.clearance_certified(x, T, G.MARGIN, self_gap, n_start, depth)
    for b in (0, 7, 20, 32):
        c1, t1 = s.clearance_certified(x[b:b + 1], T[b:b + 1], G.MARGIN, self_gap, n_start, depth)
        assert c1.tobytes() == clr[b:b + 1].tobytes() and t1.tobytes() == cert[b:b + 1].tobytes(), b
    assert len(set(clr["status"].tolist())) >= 2


# ---- 4. the moving world ----------------------------------------------------------------------------------------------------------------------
def moving_solver(M, name, obs=None, tracks=None):
    s = solver(M, name)
    ms, tables = G.moving_robot(name)
    for a, t in enumerate(tables):
        s.set_robot_spheres(t, arm=a)
    if obs is not None:
        s.set_obstacles(obs)
    if tracks is not None:
        s.set_obstacle_tracks(*tracks)
    return s, ms, tables


@pytest.mark.parametrize("per_problem", [False, True], ids=["one-world", "world-per-problem"])
@pytest.mark.parametrize("name", G.MOVING)
def test_timed_check_delay_search_and_sphere_tracks_vs_reference(M, name, per_problem):
    narm, nseg = G.shape(name)
    sx, su, sT = G.moving_plans(name)
    w, ts, margin = MW.window_of(sT), MW.start_times(sT), G.MV_MARGINS[name]
    worlds = G.moving_worlds(M, name, w, per_problem)
    s, ms, tables = moving_solver(M, name)
    s.set_bounds(MW.slow_rows(M, B))
    prof_all, rec = s.retime(sx, su, sT, N_GRID)
    s.clear_bounds()
    assert (rec["status"] == 0).all() and (prof_all[:, -1, 0] > 1.05 * sT).all()

    def set_world(ws):
        if per_problem:
            s.set_obstacles(np.ascontiguousarray(np.stack([x[0] for x in ws])))
            s.set_obstacle_tracks(np.stack([x[1][0] for x in ws]), np.ascontiguousarray(np.stack([x[1][1] for x in ws])), ws[0][1][2], ws[0][1][3])
        else:
            s.set_obstacles(ws[0][0]); s.set_obstacle_tracks(*ws[0][1])
    set_world(worlds)
    for prof, t_start in ((None, None), (prof_all, ts)):
        ref = [MW.timed_references(ms, tables, mr.World(*worlds[b]), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None if prof is None else prof[b:b + 1],
                                   None if t_start is None else t_start[b:b + 1], N_PTS, margin)[0] for b in range(B)]
        G.assert_moving_case_is_fair(ref, worlds[0][1], (name, per_problem, prof is not None))
        got = s.clearance_timed(sx, sT, prof, t_start, N_PTS, margin, 0)
        MW.check_timed_records(got, ref, sT if prof is None else prof[:, -1, 0], N_PTS, (name, per_problem, prof is not None))
    # the sphere centres on the world clock
    for prof, t_start, clock in ((None, None, (0.0, 0.1, 9)), (prof_all, ts, (-0.5, 0.13, 17))):
        got = s.sphere_tracks(sx, sT, clock[0], clock[1], clock[2], prof, t_start)
        assert got.shape == (B, sum(t.shape[0] for t in tables), clock[2], 3)
        for b in range(B):
            want = mr.sphere_tracks_reference(ms, tables, nseg, sx[b], sT[b], None if prof is None else prof[b], 0.0 if t_start is None else t_start[b], *clock)
            assert np.abs(got[b] - want).max() <= 1e-10, (name, b, np.abs(got[b] - want).max())
    # the delay search under the press
    presses = G.moving_worlds(M, name, w, per_problem, press=True)
    set_world(presses)
    delays = MW.delay_grid(G.DELAYS_K, w)
    for cw in (False, True):
        ref = [MW.delay_references(ms, tables, mr.World(*presses[b]), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None, N_PTS, delays, cw, margin)[0]
               for b in range(B)]
        G.assert_delay_case_is_fair(ref, (name, per_problem, cw))
        got, d_all = s.start_delay(sx, sT, delays, None, cw, N_PTS, margin, 0)
        MW.check_delay_records(got, d_all, ref, delays, (name, per_problem, cw))
    s.close()


def mcert_world(name, idx):
    """the obstacle sets and track table of the plans idx as Solver takes them (tests/test_gpu_moving_cert.py::world_of)"""
    d, case = G.mcert_data(name), G.MCERT_CASES[name]
    if not case.per_problem:
        return d["obs"][0], d["tracks"][0]
    tr = [d["tracks"][b] for b in idx]
    return (np.ascontiguousarray(np.stack([d["obs"][b] for b in idx])),
            (np.stack([t[0] for t in tr]), np.ascontiguousarray(np.stack([t[1] for t in tr])), tr[0][2], tr[0][3]))


@pytest.mark.parametrize("name", G.MOVING)
def test_certified_timed_vs_host_statement_and_reference(M, name):
    """general_11 in one world, dual_21 with one obstacle set and track table per problem; wait and hold positive"""
    case, d, ref = G.MCERT_CASES[name], G.mcert_data(name), G.mcert_reference(name)
    G.assert_mcert_case_is_fair(name, ref)
    idx = np.arange(MH.NP)
    obs, tracks = mcert_world(name, idx)
    s = cert_solver(M, name, MH.NP, obs, tracks)
    clr, cert = s.clearance_certified_timed(np.ascontiguousarray(d["x"]), d["T"], d["ts"], d["w"], d["h"], case.margin, case.self_gap, case.n_start,
                                            case.n_rest, case.max_depth)
    for b in range(MH.NP):
        hc, ht = G.mcert_one(M, name, b)
        H.check_records(clr[b], cert[b], dict(clr=hc, cert=ht), ("host", name, b))
        H.check_records(clr[b], cert[b], ref[b], ("reference", name, b))


# ---- 5. the two arms of dual_21 in the other order ----------------------------------------------------------------------------------------------
PX, PU = np.r_[7:14, 0:7, 21:28, 14:21], np.r_[7:14, 0:7]


def swapped_models(M):
    ms = G.models("dual_21")
    out = (M.Model * 2)(); out[0] = ms[1]; out[1] = ms[0]
    return out


def assert_same_certificates(clr, cert, clr_s, cert_s, n0, n1, what):
    """records of the arms in the other order: every integer and every time bitwise equal, the distances within the 1e-12 (1 + |x|) of
    check_records (a pair's bound subtracts its two spheres' D in the other order), the named spheres remapped"""
    back = lambda i: i - n1 if i >= n1 else i + n0          # an index of the swapped robot -> the index of the same sphere in the first robot
    for b in range(clr.shape[0]):
        tag = (what, b)
        for f in ("n_hit", "status"):
            assert clr[f][b] == clr_s[f][b], (tag, f, clr[b], clr_s[b])
        for f in ("t_min", "t_first"):
            assert clr[f][b].tobytes() == clr_s[f][b].tobytes(), (tag, f, clr[b], clr_s[b])
        for f in ("n_eval", "n_clear", "n_undecided", "depth"):
            assert cert[f][b] == cert_s[f][b], (tag, f, cert[b], cert_s[b])
        assert cert["t_lower"][b].tobytes() == cert_s["t_lower"][b].tobytes(), (tag, cert[b], cert_s[b])
        assert H.close(float(clr_s["d_min"][b]), float(clr["d_min"][b])) and H.close(float(cert_s["d_lower"][b]), float(cert["d_lower"][b])), tag
        if clr["sphere"][b] < 0:
            assert clr_s["sphere"][b] == clr["sphere"][b] and clr_s["other"][b] == clr["other"][b], tag
        elif clr["other"][b] >= 0:
            assert clr_s["other"][b] == clr["other"][b] and back(int(clr_s["sphere"][b])) == clr["sphere"][b], (tag, clr[b], clr_s[b])
        else:
            assert clr_s["other"][b] < 0, (tag, clr[b], clr_s[b])
            assert {back(int(clr_s["sphere"][b])), back(-1 - int(clr_s["other"][b]))} == {int(clr["sphere"][b]), -1 - int(clr["other"][b])}, (tag, clr[b], clr_s[b])


def test_two_different_arms_swapped(M):
    """dual_21 with the arms in the other order, and the plan columns, sphere tables and payload rows swapped to match: limits,
    clearance_certified and clearance_certified_timed give the same records up to the relabelling of arms, channels and spheres.  On twin Pandas
    this is vacuous; here a kernel that reads arm 0's model, table or payload for arm 1 anywhere fails it, whatever a reference says"""
    name = "dual_21"
    sw = swapped_models(M)
    # limits under payload rows
    c = G.reader_case(name, True)
    s = solver(M, name); s.set_bounds(c["table"]); set_payloads(s, name)
    a = s.limits(c["sx"], c["su"], c["sT"], N_PTS, TOL, c["lin_max"], c["ang_max"])
    t = solver(M, name, models=sw); t.set_bounds(c["table"]); set_payloads(t, name, swap=True)
    b_ = t.limits(np.ascontiguousarray(c["sx"][:, :, PX]), np.ascontiguousarray(c["su"][:, :, PU]), c["sT"], N_PTS, TOL, c["lin_max"], c["ang_max"])
    for f in ("excess", "t_at", "stretch", "t_first", "n_viol", "status"):
        assert a[f].tobytes() == b_[f].tobytes(), f
    ch = b_["channel"].copy()
    joint, per_arm = ch[:, :4], ch[:, 4:]
    ch[:, :4] = np.where(joint >= 0, (joint + 7) % 14, joint)
    ch[:, 4:] = np.where(per_arm >= 0, 1 - per_arm, per_arm)
    assert np.array_equal(ch, a["channel"]), (ch, a["channel"])
    assert (a["channel"][:, :4] >= 7).any() and (a["channel"][:, :4] < 7).any()          # (both arms are named)
    # the certificate
    tables = G.cert_tables(name)
    n0, n1 = tables[0].shape[0], tables[1].shape[0]
    self_gap, _, n_start, _, _ = G.CERT_CASES[name]
    _, seed, depth = G.DEEP          # (the plans of the deep case: their records name spheres of arm 1 and a pair of spheres, one of each arm)
    x, T = G.cert_plans(name, seed)
    clr, cert = cert_solver(M, name, B, G.cert_world(name)).clearance_certified(x, T, G.MARGIN, self_gap, n_start, depth)
    clr_s, cert_s = cert_solver(M, name, B, G.cert_world(name), models=sw, tables=tables[::-1]).clearance_certified(
        np.ascontiguousarray(x[:, :, PX]), T, G.MARGIN, self_gap, n_start, depth)
    assert_same_certificates(clr, cert, clr_s, cert_s, n0, n1, "certified")
    assert (clr["sphere"] >= n0).any() and (clr["other"] < 0).any()
    # ... in the moving world
    case, d = G.MCERT_CASES[name], G.mcert_data(name)
    obs, tracks = mcert_world(name, np.arange(MH.NP))
    args = (d["T"], d["ts"], d["w"], d["h"], case.margin, case.self_gap, case.n_start, case.n_rest, case.max_depth)
    clr, cert = cert_solver(M, name, MH.NP, obs, tracks).clearance_certified_timed(np.ascontiguousarray(d["x"]), *args)
    clr_s, cert_s = cert_solver(M, name, MH.NP, obs, tracks, models=sw, tables=tables[::-1]).clearance_certified_timed(
        np.ascontiguousarray(d["x"][:, :, PX]), *args)
    assert_same_certificates(clr, cert, clr_s, cert_s, n0, n1, "certified_timed")
    assert (clr["sphere"] >= n0).any() and (clr["other"] < 0).any()
    assert np.abs(d["x"][:, :, PX] - d["x"]).max() > 1e-2          # (the halves differ: the swap is visible)
