"""NumPy reference of the checks in a moving world (include/mpcmp_moving.h): tracks, the timed clearance check, the start-delay search and the
export of a plan's sphere centres.  It shares nothing with the C++.

Robot side: forward kinematics and the distances at rest from clearances_np / sphere_centres of tests/test_clearance_host.py, the samples of a plan
on its own clock from oracle_py.sample, on a retimed clock from the sampler of tests/route_retime_reference.py (a plan is a route of one leg).
Moving obstacles: the reference moves the OBSTACLE where the library moves the point: per sample it shifts a (and b of a capsule) by the track's
offset and uses d + n.p for a half-space, so a sign or frame error of the library cannot cancel against the same error here.
"""
import numpy as np

import oracle_py as o
import retime_reference as R
from route_retime_reference import sample_retimed_route_np
from test_clearance_host import clearances_np, sphere_centres


def track_np(P, t0, dt, tau):
    """offsets [..., 3] of the track P [n_key][3] on the clock t0 + k dt at the world times tau [...]: piecewise linear, held outside the keys"""
    P, tau = np.asarray(P, dtype=np.float64).reshape(-1, 3), np.asarray(tau, dtype=np.float64)
    n_key = P.shape[0]
    if n_key == 1:
        return np.broadcast_to(P[0], tau.shape + (3,)).copy()
    u = np.clip((tau - t0) / dt, 0.0, n_key - 1.0)
    k = np.minimum(np.floor(u), n_key - 2).astype(int)
    f = (u - k)[..., None]
    return (1.0 - f) * P[k] + f * P[k + 1]


def moved_clearance(ob, cen, rad, p):
    """clearances [S, nsph] of the sphere centres cen [S, nsph, 3] (radii rad) against the obstacle record `ob` MOVED by p [S, 3]: the four formulas of
    include/mpcmp.h with the obstacle's own points shifted"""
    a, b, r, kind = np.array(ob["a"], dtype=np.float64), np.array(ob["b"], dtype=np.float64), float(ob["r"]), int(ob["type"])
    if kind == 3:                                  # half-space n.x <= d, moved: n.(x - p) <= d  <=>  n.x <= d + n.p
        return cen @ a - (b[0] + p @ a)[:, None] - rad[None, :]
    am = (a[None, :] + p)[:, None, :]              # [S, 1, 3]
    if kind == 0:
        return np.linalg.norm(cen - am, axis=-1) - r - rad[None, :]
    if kind == 1:
        bm = (b[None, :] + p)[:, None, :]
        ab = bm - am
        l2 = (ab * ab).sum(axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(l2 > 0, np.clip(((cen - am) * ab).sum(axis=-1) / l2, 0.0, 1.0), 0.0)
        return np.linalg.norm(cen - am - t[..., None] * ab, axis=-1) - r - rad[None, :]
    d = np.abs(cen - am) - b[None, None, :]
    return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(d.max(axis=-1), 0.0) - r - rad[None, :]


def retimed_s(prof, T, t):
    """the "Clock" and "Retimed sample" rules of include/mpcmp_retime.h restated for ONE time t of a plan's profile [n + 1][2] = (t_k, x_k):
    lambda = sqrt(x_k) + w_k (t - t_k) / 2T,  s = s_k + (t - t_k) (sqrt(x_k) + lambda) / 2T  on the interval k with t_k <= t; the end is s = 1"""
    n = prof.shape[0] - 1
    t_k, x_k, h = prof[:, 0], prof[:, 1], 1.0 / (2.0 * T)
    if t >= t_k[n]:
        return 1.0
    k = min(max(int(np.searchsorted(t_k, t, side="right")) - 1, 0), n - 1)
    lk, w = np.sqrt(x_k[k]), (x_k[k + 1] - x_k[k]) * n
    lam = lk + w * (t - t_k[k]) * h
    return min(max(k / n + (t - t_k[k]) * (lk + lam) * h, 0.0), 1.0)


def run_time(sT, prof):
    return float(sT) if prof is None else float(prof[-1, 0])


def plan_samples(models, nseg, sx, su, sT, prof, n_pts):
    """the n_pts + 1 samples of ONE plan sx [N][14 narm] on its running clock: (t [S], q [S][7 narm])"""
    narm, N = len(models), sx.shape[0]
    if prof is None:
        q = np.zeros((n_pts + 1, 7 * narm))
        for a in range(narm):
            xa, _ = R.arm_nodes(sx, np.zeros((N, 7 * narm)), a)
            q[:, 7 * a:7 * a + 7] = o.sample(nseg, xa, np.zeros((N, 7)), sT, n_pts)[:, 1:8]
        return np.array([(i / n_pts) * sT for i in range(n_pts + 1)]), q
    rows = sample_retimed_route_np(list(models), nseg, sx[None], su[None], np.array([sT]), prof[None], n_pts)
    return rows[:, 0].copy(), np.concatenate([rows[:, 1 + 28 * a:8 + 28 * a] for a in range(narm)], axis=1)


def posture_at(nseg, sx, s):
    """q [7 narm] of the plan sx [N][14 narm] at the normalised time s"""
    nq = sx.shape[1] // 2
    return R.lagrange_np(nseg, sx[:, :nq], s)


class World:
    """obstacle records [n_obs], and tracks = None or (track_of [n_obs], offsets [n_tracks][n_key][3], t0, dt)"""
    def __init__(self, obs, tracks=None):
        self.obs, self.tracks = obs, tracks

    def tracked(self):
        if self.tracks is None:
            return []
        return [(k, int(t)) for k, t in enumerate(self.tracks[0]) if t >= 0]

    def offsets(self, trk, tau):
        _, off, t0, dt = self.tracks
        return track_np(off[trk], t0, dt, tau)


def rest_clearances(models, tables, world, q, self_gap):
    """what does not depend on the world time: (dob_rest [S, nsph, n_obs] with the tracks ignored, drb [S, nsph, nsph], centres [S, nsph, 3], radii)"""
    dob_rest, drb = clearances_np(models, tables, world.obs, q, self_gap)
    cen, rad, _, _ = sphere_centres(models, tables, q)
    return dob_rest, drb, cen, rad


def moved_columns(world, rest, tau):
    """dob [S, nsph, n_obs] at the world times tau [S]: the columns of the tracked obstacles replaced by the clearances against the moved obstacle"""
    dob_rest, _, cen, rad = rest
    dob = dob_rest.copy()
    for k, trk in world.tracked():
        dob[:, :, k] = moved_clearance(world.obs[k], cen, rad, world.offsets(trk, tau))
    return dob


def moving_clearances(models, tables, world, q, tau, self_gap):
    """every clearance of the configurations q [S, 7 narm] at the world times tau [S]: (dob [S, nsph, n_obs], drb [S, nsph, nsph], dob_rest), the last
    with the tracks ignored"""
    rest = rest_clearances(models, tables, world, q, self_gap)
    return moved_columns(world, rest, tau), rest[1], rest[0]


def _smin(dob, drb):
    S = dob.shape[0]
    return np.minimum(dob.reshape(S, -1).min(axis=1, initial=np.inf), drb.reshape(S, -1).min(axis=1, initial=np.inf))


def timed_reference(models, tables, world, q, t, T_run, t_start, n_pts, margin, self_gap):
    """the record fields of ONE plan from its samples (t [S], q [S][7 narm]) started at the world time t_start; the keys of
    test_gpu_clearance.reference, and status_rest: the status with the tracks ignored"""
    dob, drb, dob_rest = moving_clearances(models, tables, world, q, t_start + t, self_gap)
    smin, smin_rest = _smin(dob, drb), _smin(dob_rest, drb)
    hit = smin < margin
    first = int(np.argmax(hit)) if hit.any() else -1
    return dict(dob=dob, drb=drb, smin=smin, d_min=smin.min(), n_hit=int(hit.sum()), t_first=(first / n_pts) * T_run if first >= 0 else -1.0,
                status=int(hit.any()), near=bool((np.abs(smin - margin) <= 1e-9).any()), status_rest=int((smin_rest < margin).any()))


def delay_reference(models, tables, world, q, t, delays, check_wait, margin, self_gap):
    """the start-delay search of ONE plan: run k = the timed check started at delays[k], joined (check_wait) with the start posture q[0] at the
    world times delays[0 .. k].  -> d_all [K], index, n_clear, status, d_min, near (some sample or wait sample within 1e-9 of the margin)"""
    K = len(delays)
    d_run, near = np.zeros(K), False
    wait = np.zeros(K)
    rest = rest_clearances(models, tables, world, q, self_gap)
    for k in range(K):
        smin = _smin(moved_columns(world, rest, delays[k] + t), rest[1])
        d_run[k] = smin.min()
        near = near or bool((np.abs(smin - margin) <= 1e-9).any())
        wait[k] = smin[0]                          # (the start posture at the world time delays[k] is sample 0 of run k)
    d_all = np.minimum(d_run, np.minimum.accumulate(wait)) if check_wait else d_run
    clear = ~(d_all < margin)
    index = int(np.argmax(clear)) if clear.any() else -1
    return dict(d_all=d_all, index=index, n_clear=int(clear.sum()), status=0 if index >= 0 else 1, d_min=d_all[index] if index >= 0 else d_all.max(),
                delay=delays[index] if index >= 0 else -1.0, near=near)


def sphere_tracks_reference(models, tables, nseg, sx, sT, prof, t_start, t0, dt, n_key):
    """[nsph][n_key][3]: the world centres of ONE plan's spheres at the world times t0 + k dt, the plan time clamped to [0, T_run]"""
    T_run = run_time(sT, prof)
    q = np.zeros((n_key, sx.shape[1] // 2))
    for k in range(n_key):
        tp = min(max(t0 + k * dt - t_start, 0.0), T_run)
        s = (tp / T_run if T_run > 0 else 0.0) if prof is None else retimed_s(prof, sT, tp)
        q[k] = posture_at(nseg, sx, min(s, 1.0))
    cen, _, _, _ = sphere_centres(models, tables, q)
    return np.ascontiguousarray(np.transpose(cen, (1, 0, 2)))
