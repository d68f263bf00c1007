"""Two behaviours of the static clearance checks that their kernels share text with the timed ones must not lose (include/mpcmp.h, "clearance";
include/mpcmp_clearance_cert.h):

1. the track table of the context does not reach them: mpcmp_clearance_batch and mpcmp_clearance_certified_batch read the obstacles where
   mpcmp_set_obstacles put them, whatever mpcmp_set_obstacle_tracks said since;
2. the static certificate does not test sol_T: a sol_T that is not finite leaves d_min, the indices, the counts and the certificate's integers as
   they are and only makes the times non-finite, where the timed member returns the NaN records.

Shapes: one arm, num_seg 4, B = 3 seeded plans, 8 skeleton spheres, two obstacles, one of them tracked on 2 keys that carry it through the arm's
base column (which every posture occupies) while every plan runs.
"""
import numpy as np
import pytest

import moving_reference as mr
import test_clearance_cert_host as H

NSEG, B, N_PTS, SEED = 4, 3, 10, 20261021
MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
PARK = (0.0, 0.0, 5.0)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def setup(M):
    """-> (models, [table of 8 spheres], obstacles [2], tracks, sx [B][N][14], sT [B])"""
    models, _, tabs = H.robot(1)
    table = np.ascontiguousarray(tabs[0][np.linspace(0, tabs[0].shape[0] - 1, 8).astype(int)])
    obs = np.array([M.obstacle(M.OBS_SPHERE, (0.55, 0.0, 0.75), (0, 0, 0), 0.10), M.obstacle(M.OBS_SPHERE, PARK, (0, 0, 0), 0.08)], dtype=M.OBSTACLE_DTYPE)
    # the parked ball goes from x = -0.5 to x = 0.5 at the height of the first link between the world times 0 and 1: every plan lasts 1 s at least
    path = np.array([[-0.5, 0.0, 0.25], [0.5, 0.0, 0.25]])
    tracks = (np.array([-1, 0], dtype=np.int32), np.ascontiguousarray((path - np.array(PARK))[None]), 0.0, 1.0)
    sx, sT = H.plans(1, NSEG, SEED, n=B)
    return models, [table], obs, tracks, np.ascontiguousarray(sx), np.ascontiguousarray(sT)


def solver(M, table, obs):
    s = M.Solver(M.default_config(NSEG, 1, margins=MARGINS), B)
    s.set_robot_spheres(table, arm=0)
    s.set_obstacles(obs)
    return s


@pytest.mark.gpu
def test_tracks_do_not_reach_the_static_checks(M):
    models, tables, obs, tracks, sx, sT = setup(M)
    # the reference first: a test in which the track does nothing must not pass
    su = np.zeros((B, 3 * NSEG + 1, 7))
    ref = {}
    for name, wld in (("rest", mr.World(obs)), ("moving", mr.World(obs, tracks))):
        ref[name] = []
        for b in range(B):
            t, q = mr.plan_samples(models, NSEG, sx[b], su[b], sT[b], None, N_PTS)
            ref[name].append(mr.timed_reference(models, tables, wld, q, t, sT[b], 0.0, N_PTS, 0.0, 0)["d_min"])
    changed = np.abs(np.array(ref["moving"]) - np.array(ref["rest"])) > 1e-3
    print("reference d_min at rest %s, with the track %s" % (np.round(ref["rest"], 4), np.round(ref["moving"], 4)))
    assert changed.any()

    s = solver(M, tables[0], obs)
    before = s.clearance(sx, sT, N_PTS, 0.0, 0), s.clearance_certified(sx, sT, 0.0, 0, 1, 3)
    s.set_obstacle_tracks(*tracks)
    after = s.clearance(sx, sT, N_PTS, 0.0, 0), s.clearance_certified(sx, sT, 0.0, 0, 1, 3)
    assert after[0].tobytes() == before[0].tobytes()
    assert after[1][0].tobytes() == before[1][0].tobytes() and after[1][1].tobytes() == before[1][1].tobytes()
    # ... while the timed members on the same context see the ball
    timed = s.clearance_timed(sx, sT, None, None, N_PTS, 0.0, 0)
    assert np.abs(timed["d_min"] - ref["moving"]).max() <= 1e-10
    assert (np.abs(timed["d_min"] - before[0]["d_min"]) > 1e-3)[changed].all()
    cert_timed = s.clearance_certified_timed(sx, sT, None, None, None, 0.0, 0, 1, 1, 3)[0]
    assert (np.abs(cert_timed["d_min"] - before[1][0]["d_min"]) > 1e-3).any()
    s.close()


def bad_times(sT):
    T = sT.copy()
    T[1], T[2] = np.inf, np.nan
    return T


def check_static_with_bad_times(good, bad, what):
    """good / bad: (record, certificate) of one plan with its finite sol_T / with sol_T = `what`.  Everything but the times is equal; of the times,
    what the commit before the merge of the certified kernels returned, recorded here and not designed: a time that exists is the normalised time
    times sol_T, so +inf for +inf and NaN for NaN, and a time that does not exist stays -1"""
    (gc, gt), (bc, bt) = good, bad
    for f in ("sphere", "other", "n_hit", "status"):
        assert bc[f] == gc[f], (what, f)
    assert bc["d_min"].tobytes() == gc["d_min"].tobytes(), what
    for f in ("n_eval", "n_clear", "n_undecided", "depth"):
        assert bt[f] == gt[f], (what, f)
    assert bt["d_lower"].tobytes() == gt["d_lower"].tobytes(), what
    is_it = np.isnan if np.isnan(what) else (lambda v: v == np.inf)
    assert is_it(bt["t_lower"]), (what, bt["t_lower"])
    assert is_it(bc["t_min"]) if gc["sphere"] >= 0 else bc["t_min"] == -1.0, (what, bc["t_min"])
    assert is_it(bc["t_first"]) if gc["n_hit"] > 0 else bc["t_first"] == -1.0, (what, bc["t_first"])


def check_nan_records(M, clr, cert, what):
    assert clr["status"] == M.CLR_NAN and np.isnan(clr["d_min"]) and clr["t_min"] == -1.0 and clr["t_first"] == -1.0, (what, clr)
    assert clr["sphere"] == -1 and clr["other"] == 0 and clr["n_hit"] == 0, (what, clr)
    assert np.isnan(cert["d_lower"]) and cert["t_lower"] == -1.0, (what, cert)
    assert cert["n_eval"] == 0 and cert["n_clear"] == 0 and cert["n_undecided"] == 0 and cert["depth"] == 0, (what, cert)


def test_static_certificate_does_not_test_sol_T_on_the_host(M):
    models, tables, obs, tracks, sx, sT = setup(M)
    T = bad_times(sT)
    for b in (1, 2):
        good = M.clearance_certified_one(models, NSEG, tables, obs, sx[b], sT[b], 0.02, 0, 1, 3)
        bad = M.clearance_certified_one(models, NSEG, tables, obs, sx[b], T[b], 0.02, 0, 1, 3)
        check_static_with_bad_times(good, bad, T[b])
        check_nan_records(M, *M.clearance_certified_timed_one(models, NSEG, tables, obs, tracks, sx[b], T[b], 0.0, 0.0, 0.0, 0.02, 0, 1, 1, 3), T[b])
        check_nan_records(M, *M.clearance_certified_timed_one(models, NSEG, tables, obs, None, sx[b], T[b], 0.0, 0.0, 0.0, 0.02, 0, 1, 1, 3), T[b])


@pytest.mark.gpu
def test_static_certificate_does_not_test_sol_T_on_the_gpu(M):
    models, tables, obs, tracks, sx, sT = setup(M)
    T = bad_times(sT)
    s = solver(M, tables[0], obs)
    good, bad = s.clearance_certified(sx, sT, 0.02, 0, 1, 3), s.clearance_certified(sx, T, 0.02, 0, 1, 3)
    assert bad[0][0].tobytes() == good[0][0].tobytes() and bad[1][0].tobytes() == good[1][0].tobytes()       # (the plan whose sol_T stayed finite)
    for b in (1, 2):
        check_static_with_bad_times((good[0][b], good[1][b]), (bad[0][b], bad[1][b]), T[b])
        host = M.clearance_certified_one(models, NSEG, tables, obs, sx[b], T[b], 0.02, 0, 1, 3)
        for f in ("sphere", "other", "n_hit", "status"):
            assert bad[0][b][f] == host[0][f], (b, f)
    for with_tracks in (False, True):
        if with_tracks:
            s.set_obstacle_tracks(*tracks)
        clr, cert = s.clearance_certified_timed(sx, T, None, None, None, 0.02, 0, 1, 1, 3)
        assert clr["status"][0] != M.CLR_NAN
        for b in (1, 2):
            check_nan_records(M, clr[b], cert[b], (with_tracks, T[b]))
    s.close()
