"""NumPy restatement of the certified clearance rule in a moving world (include/mpcmp_moving_cert.h) that shares no code with the library.

Robot side: the forward kinematics, the four signed distances and the cubic of a joint on an interval in Bernstein form are the NumPy functions of
tests/clearance_cert_reference.py (power basis, textbook conversion matrix).  New here: the timeline of wait, motion and hold with exact rational
midpoints PER PHASE (fractions), plain Python lists for the levels, a track as an explicit polyline, and E_k by the set formula of the header over an
explicit vertex list.  The reference moves the OBSTACLE where the library moves the point (moving_reference.moved_clearance).

certified_timed_np returns the two records as dicts and `gap`, its smallest decision gap: the minimum over all decisions it took of |d_mid - margin|
and |L - margin|.  A test compares integer fields only where that gap is far above the rounding of either side.
"""
import math
from fractions import Fraction

import numpy as np

import clearance_cert_reference as R
from moving_reference import moved_clearance

HIT, NAN, UNDECIDED = 1, 2, 4
CAPACITY, SPLIT_MAX = 4096, 2048
WAIT, MOTION, HOLD = 0, 1, 2


def track_u(n_key, t0, dt, tau):
    return min(max((tau - t0) / dt, 0.0), n_key - 1.0)


def track_point(P, t0, dt, tau):
    """the polyline P [n_key][3] on the clock t0 + k dt at the world time tau, held outside its keys"""
    P = np.asarray(P, float).reshape(-1, 3)
    n_key = P.shape[0]
    if n_key == 1:
        return P[0].copy()
    u = track_u(n_key, t0, dt, tau)
    k = min(int(math.floor(u)), n_key - 2)
    f = u - k
    return (1.0 - f) * P[k] + f * P[k + 1]


def track_bound(P, t0, dt, tau_a, tau_m, tau_b):
    """(p_m, E_k, the vertex list): the offset at tau_m and the largest distance from it of the polyline's vertices on [tau_a, tau_b]"""
    P = np.asarray(P, float).reshape(-1, 3)
    n_key = P.shape[0]
    pm = track_point(P, t0, dt, tau_m)
    if n_key == 1:
        return pm, 0.0, [pm]
    ua, ub = track_u(n_key, t0, dt, tau_a), track_u(n_key, t0, dt, tau_b)
    verts = [track_point(P, t0, dt, tau_a), track_point(P, t0, dt, tau_b)] + [P[j] for j in range(int(math.ceil(ua)), int(math.floor(ub)) + 1)]
    return pm, max(float(np.linalg.norm(v - pm)) for v in verts), verts


def nan_records():
    return dict(clr=dict(d_min=np.nan, t_min=-1.0, t_first=-1.0, sphere=-1, other=0, n_hit=0, status=NAN),
                cert=dict(d_lower=np.nan, t_lower=-1.0, n_eval=0, n_clear=0, n_undecided=0, depth=0), gap=np.inf)


def certified_timed_np(models, tables, obstacles, tracks, nseg, x, T, t_start, wait, hold, margin, self_gap, n_start, n_rest, max_depth):
    """models: [(R0, p)] per arm; tables: one sphere record array per arm; obstacles: records or None; tracks: None or (track_of [n_obs], offsets
    [n_tracks][n_key][3], t0, dt); x [N][14 narm]"""
    narm, nq = len(models), 7 * len(models)
    q = np.asarray(x, float)[:, :nq]
    assert nseg * n_start + 2 * n_rest <= CAPACITY and 0 <= max_depth <= 16 and n_rest >= 1
    if not (np.isfinite(q).all() and np.isfinite([T, t_start, wait, hold]).all() and wait >= 0.0 and hold >= 0.0):
        return nan_records()
    arm = [a for a in range(narm) for _ in range(len(tables[a]))]
    sph = [s for a in range(narm) for s in tables[a]]
    jnt = [int(s["joint"]) for s in sph]
    cs = np.array([s["c"] for s in sph], float).reshape(-1, 3)
    rad = np.array([s["r"] for s in sph], float)
    nsph = len(sph)
    obs = [] if obstacles is None else list(obstacles)
    if tracks is None:
        tof, off, t0, dt = [-1] * len(obs), np.zeros((0, 1, 3)), 0.0, 1.0
    else:
        tof, off, t0, dt = [int(k) for k in tracks[0]], np.asarray(tracks[1], float), float(tracks[2]), float(tracks[3])
    reach = np.zeros((nsph, 7))
    for s in range(nsph):
        plen = np.linalg.norm(models[arm[s]][1], axis=1)
        for i in range(jnt[s] + 1):
            reach[s, i] = np.linalg.norm(cs[s]) + plen[i + 1:jnt[s] + 1].sum()
    robot_pairs = [(s, t) for s in range(nsph) for t in range(s + 1, nsph)
                   if arm[s] != arm[t] or (self_gap > 0 and abs(jnt[s] - jnt[t]) >= self_gap)]
    ps_, pt_ = np.array([p[0] for p in robot_pairs], int), np.array([p[1] for p in robot_pairs], int)

    # the phases in time order: (kind, level-0 count, record time of the start, duration)
    phases = ([(WAIT, n_rest, 0.0, wait)] if wait > 0.0 else []) + [(MOTION, nseg * n_start, wait, T)] + ([(HOLD, n_rest, wait + T, hold)] if hold > 0.0 else [])
    tau0 = t_start - wait

    def clock(key):
        """record time of (phase number, fraction of the phase)"""
        _, _, base, length = phases[key[0]]
        return base + float(key[1]) * length

    best = (np.inf, None)               # (d, ((phase number, fraction), sphere, robot, index))
    lower = (np.inf, None)              # (L, (phase number, fraction))
    hits, n_clear, n_und, n_eval, depth, gap = [], 0, 0, 0, 0, np.inf
    level = [(pn, i) for pn, ph in enumerate(phases) for i in range(ph[1])]          # (phase number, index inside the phase)
    l = 0
    while level:
        depth = l
        nxt, n_split = [], 0
        for pn, i in level:
            kind, n_p, base, length = phases[pn]
            den = n_p * 2 ** l
            fm = Fraction(2 * i + 1, 2 * den)
            tkey = (pn, fm)
            ta, tm, tb = base + float(Fraction(i, den)) * length, base + float(fm) * length, base + float(Fraction(i + 1, den)) * length
            if kind == MOTION:
                seg = i // (n_start * 2 ** l)
                xa, xb = 2.0 * (i / den * nseg - seg) - 1.0, 2.0 * ((i + 1) / den * nseg - seg) - 1.0
                ctrl, qm = R.bezier_of_interval(q[3 * seg:3 * seg + 4], xa, xb)
                dev = np.abs(ctrl - qm[None]).max(axis=0)
            else:
                qm, dev = q[0 if kind == WAIT else -1].copy(), np.zeros(nq)
            cen = np.zeros((nsph, 3))
            for a in range(narm):
                Rs, ps = R.frames(models[a], qm[7 * a:7 * a + 7])
                for s in range(nsph):
                    if arm[s] == a:
                        cen[s] = ps[jnt[s]] + Rs[jnt[s]] @ cs[s]
            D = np.array([reach[s] @ dev[7 * arm[s]:7 * arm[s] + 7] for s in range(nsph)])
            moved = [track_bound(off[k], t0, dt, tau0 + ta, tau0 + tm, tau0 + tb)[:2] for k in range(off.shape[0])]
            d_mid, L = np.inf, np.inf
            cand = []
            if obs and nsph:
                cols, slack = [], []
                for o, ob in enumerate(obs):
                    k = tof[o] if 0 <= tof[o] < off.shape[0] else -1
                    if k >= 0:
                        cols.append(moved_clearance(ob, cen[None], rad, moved[k][0][None])[0])
                        slack.append(moved[k][1])
                    else:
                        cols.append(R.signed_distance(ob, cen) - rad)
                        slack.append(None)
                dob = np.stack(cols, axis=1)                                  # [nsph][n_obs]
                bound = np.stack([cols[o] - D if slack[o] is None else cols[o] - D - slack[o] for o in range(len(obs))], axis=1)
                d_mid, L = min(d_mid, dob.min()), min(L, bound.min())
                s, o = np.unravel_index(np.argmin(dob), dob.shape)          # (row-major: the lowest sphere, then the lowest obstacle)
                cand.append((dob[s, o], (tkey, int(s), 0, int(o))))
            if robot_pairs:
                drb = np.linalg.norm(cen[ps_] - cen[pt_], axis=1) - rad[ps_] - rad[pt_]
                d_mid, L = min(d_mid, drb.min()), min(L, (drb - D[ps_] - D[pt_]).min())
                k = int(np.argmin(drb))                                     # (the pair list is ordered by s, then t)
                cand.append((drb[k], (tkey, int(ps_[k]), 1, int(pt_[k]))))
            for d, key in cand:
                if d < best[0] or (d == best[0] and key < best[1]):
                    best = (d, key)
            n_eval += 1
            gap = min(gap, abs(d_mid - margin))
            if d_mid < margin:
                what = "hit"
            else:
                gap = min(gap, abs(L - margin))
                if L >= margin:
                    what = "clear"
                elif l == max_depth:
                    what = "undecided"
                elif n_split < SPLIT_MAX:
                    n_split += 1
                    nxt += [(pn, 2 * i), (pn, 2 * i + 1)]
                    continue
                else:
                    what = "undecided"
            if what == "hit":
                hits.append(tkey)
            elif what == "clear":
                n_clear += 1
            else:
                n_und += 1
            if L < lower[0] or (L == lower[0] and (lower[1] is None or tkey < lower[1])):
                lower = (L, tkey)
        level = nxt
        l += 1
    clr = dict(d_min=best[0], n_hit=len(hits), t_first=clock(min(hits)) if hits else -1.0, status=(HIT if hits else 0) | (UNDECIDED if n_und else 0))
    if best[1] is None:
        clr.update(t_min=-1.0, sphere=-1, other=0)
    else:
        tkey, s, robot, idx = best[1]
        clr.update(t_min=clock(tkey), sphere=s, other=-1 - idx if robot else idx)
    cert = dict(d_lower=lower[0], t_lower=clock(lower[1]), n_eval=n_eval, n_clear=n_clear, n_undecided=n_und, depth=depth)
    return dict(clr=clr, cert=cert, gap=gap)
