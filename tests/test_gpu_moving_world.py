"""Clearance in a moving world on the GPU (include/mpcmp_moving.h: mpcmp_clearance_timed_batch*, mpcmp_start_delay_batch*,
mpcmp_sphere_tracks_batch*, the track setters) against the NumPy reference of tests/moving_reference.py, which moves the OBSTACLE where the kernels
move the point.  Plans, scene, margin, profiles and the comparison helpers are those of tests/test_moving_world_host.py (see its docstring for the
bounds: d_min 1e-10, tie-robust pair and sample, exact counts and indices away from the margin) and the fairness conditions it asserts on the
reference in every parity case.  B = 32 throughout.
"""
import numpy as np
import pytest

import moving_reference as mr
from test_gpu_clearance import MARGIN, MARGINS, check_records, reference, sampled_q, world
from test_moving_world_host import (B, MV_MARGIN, assert_fair, assert_fair_delays, check_delay_records, check_timed_records, delay_grid, delay_references,
                                    moving_world, plans, robot, slow_rows, start_times, timed_references, window_of)

pytestmark = pytest.mark.gpu
EINVAL = -1
# num_seg 4 and 8 for one arm and for two; a two-arm context exists for num_seg 6 and 8 only (mpcmp_create_multi refuses 4), so its smaller case is 6
SHAPES = [(4, 1), (8, 1), (6, 2), (8, 2)]


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def solver(M, narm, nseg, obs=None, max_batch=B):
    models, tables = robot(M, narm)
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    for a in range(narm):
        s.set_robot_spheres(tables[a], arm=a)
    if obs is not None:
        s.set_obstacles(obs)
    return s, models, tables


_PROFILES = {}


def gpu_profiles(M, s, narm, nseg):
    """the plans retimed on the GPU under rows at 45 % of the velocity limits: T_new != sol_T for every plan"""
    if (narm, nseg) not in _PROFILES:
        sx, su, sT = plans(narm, nseg)
        s.set_bounds(slow_rows(M))
        prof, rec = s.retime(sx, su, sT, 64)
        s.clear_bounds()
        assert (rec["status"] == 0).all() and (prof[:, -1, 0] > 1.05 * sT).all()
        _PROFILES[(narm, nseg)] = prof
    return _PROFILES[(narm, nseg)]


# ---- 1. static equivalence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 50])
@pytest.mark.parametrize("nseg,narm", SHAPES)
def test_a_world_at_rest_gives_the_records_of_the_static_check(M, nseg, narm, n_pts):
    obs = world(M, narm)
    s, models, tables = solver(M, narm, nseg, obs)
    sx, su, sT = plans(narm, nseg)
    ref = reference(models, tables, obs, sampled_q(narm, nseg, sx, sT, n_pts), sT, n_pts, MARGIN, 0)
    static = s.clearance(sx, sT, n_pts, MARGIN, 0)
    check_records(static, ref, sT, n_pts, "static")
    for what in ("no tracks", "every track_of -1"):
        if what != "no tracks":
            s.set_obstacle_tracks(np.full(obs.shape[0], -1), np.ones((2, 3, 3)), 0.0, 0.1)
        got = s.clearance_timed(sx, sT, None, None, n_pts, MARGIN, 0)
        check_records(got, ref, sT, n_pts, what)
        assert np.abs(got["d_min"] - static["d_min"]).max() <= 1e-10
        for b in range(B):
            if not ref[b]["near"]:
                assert all(got[f][b] == static[f][b] for f in ("t_first", "n_hit", "status")), (what, b, got[b], static[b])
        assert (got["t_min"] == static["t_min"]).sum() >= B - 1          # (a tie within rounding may name another sample)
    s.close()


# ---- 2. parity of the timed check ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_key", [1, 2, 17])
@pytest.mark.parametrize("n_pts", [1, 50, 257])
@pytest.mark.parametrize("nseg,narm", SHAPES)
def test_timed_check_matches_the_reference(M, nseg, narm, n_pts, n_key):
    sx, su, sT = plans(narm, nseg)
    obs, tracks = moving_world(M, narm, n_key, window_of(sT))
    s, models, tables = solver(M, narm, nseg, obs)
    s.set_obstacle_tracks(*tracks)
    wld = mr.World(obs, tracks)
    prof_all, ts = gpu_profiles(M, s, narm, nseg), start_times(sT)
    if n_key > 1:        # some samples fall before the first key and some after the last
        tau_lo, tau_hi = 0.0, float((ts + prof_all[:, -1, 0]).max())
        assert tau_lo < tracks[2] and tau_hi > tracks[2] + (n_key - 1) * tracks[3]
    for prof in (None, prof_all):
        for t_start in (None, ts):
            tag = (nseg, narm, n_pts, n_key, prof is not None, t_start is not None)
            ref = timed_references(models, tables, wld, nseg, sx, su, sT, prof, t_start, n_pts, MV_MARGIN, key=("gpu", nseg, narm, n_pts, prof is not None))
            assert_fair(ref, tag)
            got = s.clearance_timed(sx, sT, prof, t_start, n_pts, MV_MARGIN, 0)
            print("%s: %d of %d hit, %d changed by the tracks, max |d_min - ref| = %.2e" % (
                tag, sum(r["status"] for r in ref), B, sum(r["status"] != r["status_rest"] for r in ref),
                max(abs(g["d_min"] - r["d_min"]) for g, r in zip(got, ref))))
            check_timed_records(got, ref, sT if prof is None else prof[:, -1, 0], n_pts, tag)
    s.close()


def test_timed_check_with_pairs_inside_one_arm_and_one_world_per_problem(M):
    """self_gap 3 on thin spheres (the pair set of test_gpu_clearance), and set b of the obstacles AND of the tracks for problem b"""
    nseg, narm, n_pts = 4, 1, 50
    sx, su, sT = plans(narm, nseg)
    models, _ = robot(M, narm)
    tables = [M.link_spheres(models[0], 0.03, 0.08)]
    obs, (tof, off, t0, dt) = moving_world(M, narm, 17, window_of(sT))
    shift = np.linspace(-0.2, 0.2, B)                    # set b: the tracked obstacles pass `shift[b]` further along y
    offs = np.stack([off + np.array([0.0, shift[b], 0.0]) * (np.arange(4) < 3)[:, None, None] for b in range(B)])
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B)
    s.set_robot_spheres(tables[0])
    s.set_obstacles(np.broadcast_to(obs, (B, obs.shape[0])))
    s.set_obstacle_tracks(np.broadcast_to(tof, (B, tof.shape[0])), offs, t0, dt)
    got = s.clearance_timed(sx, sT, None, None, n_pts, 0.0, 3)
    ref = [timed_references(models, tables, mr.World(obs, (tof, offs[b], t0, dt)), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None, None, n_pts, 0.0, 3)[0]
           for b in range(B)]
    assert sum(r["near"] for r in ref) <= 0.02 * B
    # (a check of the reference alone: a kernel that read set 0 for every problem would be found out)
    ref0 = [timed_references(models, tables, mr.World(obs, (tof, offs[0], t0, dt)), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None, None, n_pts, 0.0, 3)[0]
            for b in range(B)]
    assert sum(abs(r["d_min"] - r0["d_min"]) > 1e-6 for r, r0 in zip(ref, ref0)) >= B / 4
    check_timed_records(got, ref, sT, n_pts, "self_gap 3, sets")
    s.close()


# ---- 3. parity of the delay search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 33])
@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_delay_search_matches_the_reference(M, nseg, narm, K):
    n_pts = 50
    sx, su, sT = plans(narm, nseg)
    w = window_of(sT)
    obs, tracks = moving_world(M, narm, 17, w, press=True)
    s, models, tables = solver(M, narm, nseg, obs)
    s.set_obstacle_tracks(*tracks)
    wld = mr.World(obs, tracks)
    delays = delay_grid(K, w)
    for prof in ((None, gpu_profiles(M, s, narm, nseg)) if K == 33 else (None,)):
        refs = {cw: delay_references(models, tables, wld, nseg, sx, su, sT, prof, n_pts, delays, cw, MV_MARGIN) for cw in (False, True)}
        for cw in (False, True):
            tag = (nseg, narm, K, prof is not None, cw)
            assert_fair_delays(refs[cw], refs[not cw], K, tag)
            got, d_all = s.start_delay(sx, sT, delays, prof, cw, n_pts, MV_MARGIN, 0)
            print("%s: index > 0 for %d, none for %d, max |d - ref| = %.2e" % (tag, (got["index"] > 0).sum(), (got["index"] < 0).sum(),
                                                                             max(np.abs(d_all[b] - refs[cw][b]["d_all"]).max() for b in range(B))))
            check_delay_records(got, d_all, refs[cw], delays, tag)
            bare, none = s.start_delay(sx, sT, delays, prof, cw, n_pts, MV_MARGIN, 0, all_minima=False)          # (d_min_all == NULL)
            assert none is None and bare.tobytes() == got.tobytes()
            # the timed check started at the delay found is clear
            found = got["index"] >= 0
            again = s.clearance_timed(sx, sT, prof, np.where(found, got["delay"], 0.0), n_pts, MV_MARGIN, 0)
            assert (again["status"][found] == 0).all()
            if not cw and found.any():          # (without the wait a run's minimum is that of the timed check)
                assert np.abs(again["d_min"][found] - d_all[found, got["index"][found]]).max() <= 1e-10
    s.close()


# ---- 4. sphere tracks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_sphere_tracks_match_the_reference(M, nseg, narm):
    sx, su, sT = plans(narm, nseg)
    s, models, tables = solver(M, narm, nseg)
    ts = start_times(sT)
    prof_all = gpu_profiles(M, s, narm, nseg)
    for prof, t_start, (t0, dt, n_key) in ((None, None, (0.0, 0.1, 33)), (prof_all, ts, (-0.5, 0.13, 47)), (None, ts, (1.0, 1.0, 1))):
        got = s.sphere_tracks(sx, sT, t0, dt, n_key, prof, t_start)
        assert got.shape == (B, sum(t.shape[0] for t in tables), n_key, 3)
        for b in range(B):
            ref = mr.sphere_tracks_reference(models, tables, nseg, sx[b], sT[b], None if prof is None else prof[b],
                                             0.0 if t_start is None else t_start[b], t0, dt, n_key)
            assert np.abs(got[b] - ref).max() <= 1e-10, (prof is not None, b, np.abs(got[b] - ref).max())
        # held at the first posture before the start and at the last after the end
        if n_key > 1:
            T_run = sT if prof is None else prof[:, -1, 0]
            start = np.zeros(B) if t_start is None else t_start
            k = np.arange(n_key)
            for b in range(0, B, 7):
                before, after = t0 + k * dt <= start[b], t0 + k * dt >= start[b] + T_run[b]
                assert before.any() and after.any()
                assert (got[b][:, before] == got[b][:, before][:, :1]).all() and (got[b][:, after] == got[b][:, after][:, -1:]).all()
    s.close()


def test_one_robot_plan_is_the_other_robot_moving_world(M):
    """robot A (a Panda at the second base of DUAL_BASES) exports its plans as tracks on the device; they become robot B's world through the _device
    setter, set b for problem b, and B's timed check is compared with the reference built from A's REFERENCE centres"""
    import torch
    nseg, n_pts, n_key = 4, 50, 64
    sx, su, sT = plans(1, nseg)
    model_a = M.arm_models(M.DUAL_BASES)[1]
    table_a = M.link_spheres(model_a, 0.06, 0.08)
    na = table_a.shape[0]
    A = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B, model=model_a)
    A.set_robot_spheres(table_a)
    order = np.roll(np.arange(B), 5)                     # A runs plan order[b] beside B's plan b
    ax, aT = np.ascontiguousarray(sx[order]), np.ascontiguousarray(sT[order])
    a_start = 0.3
    horizon = float(max(sT.max(), a_start + aT.max()))
    dt = horizon / (n_key - 1)
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    dx, dT = torch.from_numpy(ax).to(dev), torch.from_numpy(aT).to(dev)
    dts = torch.full((B,), a_start, dtype=torch.float64, device=dev)
    dtracks = torch.zeros((B, na, n_key, 3), dtype=torch.float64, device=dev)
    A.sphere_tracks_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, dts.data_ptr(), 0.0, dt, n_key, dtracks.data_ptr(), stream=stream)
    # B: the static world, then A's spheres at the origin, one obstacle set and one track table per problem
    models, tables = robot(M, 1)
    still = world(M, 1)
    mine = np.array([M.obstacle(M.OBS_SPHERE, (0, 0, 0), (0, 0, 0), float(r)) for r in table_a["r"]], dtype=M.OBSTACLE_DTYPE)
    obs = np.concatenate([still, mine])
    tof = np.concatenate([np.full(still.shape[0], -1), np.arange(na)]).astype(np.int32)
    Bs = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B)
    Bs.set_robot_spheres(tables[0])
    Bs.set_obstacles(np.broadcast_to(obs, (B, obs.shape[0])))
    dtof = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(tof, (B, tof.shape[0])))).to(dev)
    Bs.set_obstacle_tracks_device(B, obs.shape[0], dtof.data_ptr(), na, n_key, 0.0, dt, dtracks.data_ptr(), stream=stream)
    bx, bT = torch.from_numpy(sx).to(dev), torch.from_numpy(sT).to(dev)
    dout = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    Bs.clearance_timed_device(B, bx.data_ptr(), bT.data_ptr(), 0, 0, 0, n_pts, MARGIN, 0, dout.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = np.frombuffer(dout.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)
    ref, decided = [], 0          # (decided: A's spheres hold the reference minimum)
    for b in range(B):
        centres = mr.sphere_tracks_reference([model_a], [table_a], nseg, ax[b], aT[b], None, a_start, 0.0, dt, n_key)
        assert np.abs(dtracks[b].cpu().numpy() - centres).max() <= 1e-10
        r = timed_references(models, tables, mr.World(obs, (tof, centres, 0.0, dt)), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None, None, n_pts,
                             MARGIN)[0]
        decided += bool(r["dob"][:, :, still.shape[0]:].min() <= r["d_min"])
        ref.append(r)
    assert sum(r["near"] for r in ref) <= 0.02 * B and decided >= B / 8, decided
    check_timed_records(got, ref, sT, n_pts, "two robots")
    A.close(); Bs.close()


# ---- 5. independence of the batch -----------------------------------------------------------------------------------------------------------------
def test_records_do_not_depend_on_the_batch(M):
    nseg, narm, n_pts = 8, 2, 50
    sx, su, sT = plans(narm, nseg)
    w = window_of(sT)
    obs, tracks = moving_world(M, narm, 17, w, press=True)
    s, models, tables = solver(M, narm, nseg, obs)
    s.set_obstacle_tracks(*tracks)
    prof, ts, delays = gpu_profiles(M, s, narm, nseg), start_times(sT), delay_grid(33, w)
    clr = s.clearance_timed(sx, sT, prof, ts, n_pts, MV_MARGIN, 0)
    sd, d_all = s.start_delay(sx, sT, delays, prof, True, n_pts, MV_MARGIN, 0)
    trk = s.sphere_tracks(sx, sT, 0.0, 0.1, 20, prof, ts)
    perm = np.random.default_rng(3).permutation(B)
    c2 = s.clearance_timed(sx[perm], sT[perm], prof[perm], ts[perm], n_pts, MV_MARGIN, 0)
    s2, d2 = s.start_delay(sx[perm], sT[perm], delays, prof[perm], True, n_pts, MV_MARGIN, 0)
    t2 = s.sphere_tracks(sx[perm], sT[perm], 0.0, 0.1, 20, prof[perm], ts[perm])
    assert c2.tobytes() == clr[perm].tobytes() and s2.tobytes() == sd[perm].tobytes() and d2.tobytes() == d_all[perm].tobytes()
    assert t2.tobytes() == trk[perm].tobytes()
    for b in (0, 13, B - 1):
        one = slice(b, b + 1)
        assert s.clearance_timed(sx[one], sT[one], prof[one], ts[one], n_pts, MV_MARGIN, 0).tobytes() == clr[one].tobytes()
        s1, d1 = s.start_delay(sx[one], sT[one], delays, prof[one], True, n_pts, MV_MARGIN, 0)
        assert s1.tobytes() == sd[one].tobytes() and d1.tobytes() == d_all[one].tobytes()
        assert s.sphere_tracks(sx[one], sT[one], 0.0, 0.1, 20, prof[one], ts[one]).tobytes() == trk[one].tobytes()
    s.close()


# ---- 6. boundary cases ------------------------------------------------------------------------------------------------------------------------------
def test_rejections_write_nothing(M):
    from mpc_motion_planner_amd.capi import host
    nseg, narm = 4, 1
    sx, su, sT = plans(narm, nseg)
    obs, (tof, off, t0, dt) = moving_world(M, narm, 3, 1.0)
    s, _, _ = solver(M, narm, nseg, obs)
    L, ctx = M.lib(), s._ctx
    s.set_obstacle_tracks(tof, off, t0, dt)
    before = s.clearance_timed(sx, sT, None, None, 10, MV_MARGIN, 0)
    bad_tof = tof.copy(); bad_tof[6] = 4
    bad_off = off.copy(); bad_off[0, 0, 0] = np.nan
    for what, a in (("fewer obstacles", (1, 7, tof, 4, 3, t0, dt, off)), ("two sets", (2, 8, np.tile(tof, 2), 4, 3, t0, dt, np.tile(off, (2, 1, 1, 1)))),
                    ("track_of 4", (1, 8, bad_tof, 4, 3, t0, dt, off)), ("offset NaN", (1, 8, tof, 4, 3, t0, dt, bad_off)),
                    ("dt 0", (1, 8, tof, 4, 3, t0, 0.0, off)), ("t0 inf", (1, 8, tof, 4, 3, np.inf, dt, off)), ("65 tracks", (1, 8, tof, 65, 3, t0, dt, off)),
                    ("1025 keys", (1, 8, tof, 4, 1025, t0, dt, off)), ("no offsets", (1, 8, tof, 4, 3, t0, dt, None))):
        n_sets, n_obs, t, n_tracks, n_key, a0, ad, o = a
        rc = L.mpcmp_set_obstacle_tracks(ctx, n_sets, n_obs, host(np.ascontiguousarray(t, dtype=np.int32)), n_tracks, n_key, float(a0), float(ad),
                                         None if o is None else host(np.ascontiguousarray(o)))
        assert rc == EINVAL, what
        assert s.clearance_timed(sx, sT, None, None, 10, MV_MARGIN, 0).tobytes() == before.tobytes(), what          # (the table in force is untouched)
    out = np.zeros(B, dtype=M.START_DELAY_DTYPE); out["n_clear"] = 77
    d_all = np.full((B, 4), -7.0)
    for what, delays, K in (("unsorted", [0.0, 1.0, 0.5], 3), ("negative", [-0.5, 0.0, 1.0], 3), ("NaN", [0.0, np.nan, 1.0], 3), ("K 0", [0.0], 0),
                            ("K 257", np.arange(257.0), 257), ("no delays", None, 3)):
        d = None if delays is None else np.ascontiguousarray(delays, dtype=np.float64)
        rc = L.mpcmp_start_delay_batch(ctx, B, host(sx), host(sT), 0, None, K, None if d is None else host(d), 0, 10, 0.0, 0, host(d_all), host(out))
        assert rc == EINVAL and (out["n_clear"] == 77).all() and (d_all == -7.0).all(), what
    clr = np.zeros(B, dtype=M.CLEARANCE_DTYPE); clr["n_hit"] = 77
    for what, kw in (("B 0", dict(B=0)), ("n_pts 0", dict(n_pts=0)), ("n_pts 4097", dict(n_pts=4097)), ("margin NaN", dict(margin=np.nan)),
                     ("self_gap -1", dict(self_gap=-1)), ("n_grid 0 with a profile", dict(prof=np.ones((B, 2, 2)), n_grid=0)),
                     ("n_grid 4097", dict(prof=np.ones((B, 2, 2)), n_grid=4097))):
        a = dict(B=B, n_grid=0, prof=None, n_pts=10, margin=0.0, self_gap=0)
        a.update(kw)
        rc = L.mpcmp_clearance_timed_batch(ctx, a["B"], host(sx), host(sT), a["n_grid"], None if a["prof"] is None else host(a["prof"]), None, a["n_pts"],
                                           float(a["margin"]), a["self_gap"], host(clr))
        assert rc == EINVAL and (clr["n_hit"] == 77).all(), what
    trk = np.full((B, 24, 2, 3), -7.0)
    for what, (a0, ad, n_key) in (("dt 0", (0.0, 0.0, 2)), ("n_key 0", (0.0, 0.1, 0)), ("n_key 1025", (0.0, 0.1, 1025)), ("t0 NaN", (np.nan, 0.1, 2))):
        assert L.mpcmp_sphere_tracks_batch(ctx, B, host(sx), host(sT), 0, None, None, float(a0), float(ad), n_key, host(trk)) == EINVAL, what
        assert (trk == -7.0).all(), what
    # more problems than obstacle sets (sets of obstacles and of tracks, 16 of each)
    s.set_obstacles(np.broadcast_to(obs, (16, obs.shape[0])))
    s.set_obstacle_tracks(np.broadcast_to(tof, (16, 8)), np.broadcast_to(off, (16,) + off.shape), t0, dt)
    assert s.clearance_timed(sx[:16], sT[:16], None, None, 10, MV_MARGIN, 0).tobytes() == before[:16].tobytes()
    assert L.mpcmp_clearance_timed_batch(ctx, B, host(sx), host(sT), 0, None, None, 10, 0.0, 0, host(clr)) == EINVAL and (clr["n_hit"] == 77).all()
    assert L.mpcmp_start_delay_batch(ctx, B, host(sx), host(sT), 0, None, 1, host(np.zeros(1)), 0, 10, 0.0, 0, None, host(out)) == EINVAL
    assert (out["n_clear"] == 77).all()
    s.close()


def test_nan_plans_profiles_and_a_world_made_static_again(M):
    nseg, narm, n_pts = 4, 1, 50
    sx, su, sT = plans(narm, nseg)
    obs, tracks = moving_world(M, narm, 17, window_of(sT))
    s, models, tables = solver(M, narm, nseg, obs)
    s.set_obstacle_tracks(*tracks)
    prof = gpu_profiles(M, s, narm, nseg).copy()
    good = s.clearance_timed(sx, sT, prof, None, n_pts, MV_MARGIN, 0)
    bx, bT, bp, bs = sx.copy(), sT.copy(), prof.copy(), np.zeros(B)
    bx[3, 5, 2] = np.nan; bT[7] = np.inf; bp[11] = np.nan; bs[13] = np.nan          # (a failed retime leaves a profile of NaN)
    got = s.clearance_timed(bx, bT, bp, bs, n_pts, MV_MARGIN, 0)
    sd, d_all = s.start_delay(bx, bT, np.array([0.0, 0.5]), bp, True, n_pts, MV_MARGIN, 0)
    sd_good, _ = s.start_delay(sx, sT, np.array([0.0, 0.5]), prof, True, n_pts, MV_MARGIN, 0)
    trk = s.sphere_tracks(bx, bT, 0.0, 0.5, 4, bp, bs)
    for b in range(B):
        if b in (3, 7, 11, 13):
            g = got[b]
            assert g["status"] == M.CLR_NAN and np.isnan(g["d_min"]) and g["t_min"] == -1.0 and g["t_first"] == -1.0 and g["sphere"] == -1 and g["n_hit"] == 0
            assert np.isnan(trk[b]).all()
            if b != 13:          # (the delay search takes no t_start)
                assert sd[b]["status"] == M.CLR_NAN and sd[b]["index"] == -1 and sd[b]["delay"] == -1.0 and np.isnan(d_all[b]).all()
        else:
            assert got[b].tobytes() == good[b].tobytes() and sd[b].tobytes() == sd_good[b].tobytes() and np.isfinite(trk[b]).all()
    # mpcmp_set_obstacles after the tracks: the world stands still where it is parked
    s.set_obstacles(obs)
    rest = s.clearance_timed(sx, sT, None, None, n_pts, MV_MARGIN, 0)
    assert np.abs(rest["d_min"] - s.clearance(sx, sT, n_pts, MV_MARGIN, 0)["d_min"]).max() <= 1e-10
    ref = timed_references(models, tables, mr.World(obs), nseg, sx, su, sT, None, None, n_pts, MV_MARGIN)
    check_timed_records(rest, ref, sT, n_pts, "static again")
    assert sum(r["status"] for r in ref) < sum(int(g["status"] == 1) for g in good)
    # ... and removing the tracks does the same
    s.set_obstacle_tracks(*tracks)
    s.clear_obstacle_tracks()
    assert s.clearance_timed(sx, sT, None, None, n_pts, MV_MARGIN, 0).tobytes() == rest.tobytes()
    s.close()


def test_planner_facade_and_the_cpp_shim(M, tmp_path):
    """BatchMotionPlanner.check_clearance_timed / first_clear_start / plan_as_moving_world on solved moves, and examples/moving_world_selftest.cpp"""
    import json
    import os
    import subprocess
    from mpc_motion_planner_amd import scenarios
    n = 8
    pa, pb = M.BatchMotionPlanner(max_batch=n, num_seg=4, sqp_iters=3), M.BatchMotionPlanner(max_batch=n, num_seg=4, sqp_iters=3)
    x0, xf = scenarios.make_batch(n, MARGINS)
    for p in (pa, pb):
        p.set_constraint_margins(*MARGINS)
        p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
        p.solve_trajectory()
    floor = np.array([M.obstacle(M.OBS_HALFSPACE, (0, 0, 1.0), (-0.5, 0, 0))], dtype=M.OBSTACLE_DTYPE)
    tracks = pa.plan_as_moving_world(pb, floor, t_start=0.0, n_key=32)
    assert tracks.shape == (n, 24, 32, 3) and np.isfinite(tracks).all()
    same = pb.check_clearance_timed(0.0, 100, 0.0)          # B runs A's own plans at the same time: the two robots coincide all the way
    assert (same["status"] == 1).all() and (same["d_min"] <= -0.12 + 1e-9).all() and (same["other"] >= 1).all()
    sd, d_all = pb.first_clear_start(np.array([0.0, 100.0]), True, 100, 0.0)
    assert d_all.shape == (n, 2) and (sd["index"] != 0).all()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "moving_world_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "moving_world_selftest.cpp"), "-L" + os.path.join(root, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(root, "mpc_motion_planner_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["still_status"] == 0 and rec["moving_d_min"] <= rec["still_d_min"] and rec["reset_d_min"] == rec["still_d_min"]
    assert rec["index"] < 0 or rec["again_status"] == 0
