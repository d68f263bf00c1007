"""NumPy restatement of the certified clearance rule (include/mpcmp_clearance_cert.h) that shares no code with the library: its own forward
kinematics from the model arrays, the four signed distances written out, the cubic of a joint on an interval in POWER basis (numpy.polynomial:
the segment's cubic through its four nodes, re-expanded about the interval's start and scaled to [0, 1]) and converted to Bernstein form by the
textbook matrix, exact rational midpoints for every order of times, and a level loop on plain lists.

certified_np returns the two records as dicts and `gap`, its smallest decision gap: the minimum over all decisions it took of |d_mid - margin| and
|L - margin|.  A test compares integer fields only where that gap is far above the rounding of either side.
"""
from fractions import Fraction

import numpy as np
from numpy.polynomial import polynomial as P

HIT, NAN, UNDECIDED = 1, 2, 4
CAPACITY, SPLIT_MAX = 4096, 2048
XI = np.array([-1.0, -0.5, 0.5, 1.0])
# Bernstein control points of a cubic a0 + a1 u + a2 u^2 + a3 u^3 on [0, 1]
POWER_TO_BERNSTEIN = np.array([[1.0, 0.0, 0.0, 0.0], [1.0, 1.0 / 3.0, 0.0, 0.0], [1.0, 2.0 / 3.0, 1.0 / 3.0, 0.0], [1.0, 1.0, 1.0, 1.0]])


def model_arrays(mdl):
    """(R0 [7][3][3], p [7][3]) of a ctypes Model"""
    return (np.array([list(mdl.R0[i]) for i in range(7)]).reshape(7, 3, 3), np.array([list(mdl.p[i]) for i in range(7)]))


def frames(model, q):
    """world rotation [7][3][3] and origin [7][3] of the joint frames: p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i)"""
    R0, p = model
    Rw, pw = np.eye(3), np.zeros(3)
    Rs, ps = np.zeros((7, 3, 3)), np.zeros((7, 3))
    for i in range(7):
        c, s = np.cos(q[i]), np.sin(q[i])
        pw = pw + Rw @ p[i]
        Rw = Rw @ R0[i] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        Rs[i], ps[i] = Rw, pw
    return Rs, ps


def signed_distance(ob, x):
    """x [n][3] against one obstacle record (type, a, b, r)"""
    a, b, r = np.asarray(ob["a"], float), np.asarray(ob["b"], float), float(ob["r"])
    kind = int(ob["type"])
    if kind == 0:
        return np.linalg.norm(x - a, axis=1) - r
    if kind == 1:
        e = b - a
        l2 = e @ e
        t = np.clip((x - a) @ e / l2, 0.0, 1.0) if l2 > 0.0 else np.zeros(x.shape[0])
        return np.linalg.norm(x - a - t[:, None] * e, axis=1) - r
    if kind == 2:
        d = np.abs(x - a) - b
        return np.linalg.norm(np.maximum(d, 0.0), axis=1) + np.minimum(d.max(axis=1), 0.0) - r
    return x @ a - b[0]


def position(nseg, nodes, t):
    """the node interpolant of every column of nodes [N][c] at the normalised time t: the cubic Lagrange form on the segment of t"""
    nodes = np.asarray(nodes, float)
    seg = min(max(int(np.floor(t * nseg)), 0), nseg - 1)
    xx = 2.0 * (t * nseg - seg) - 1.0
    w = [np.prod([(xx - XI[k]) / (XI[j] - XI[k]) for k in range(4) if k != j]) for j in range(4)]
    return sum(w[j] * nodes[3 * seg + j] for j in range(4))


def bezier_of_interval(nodes4, xa, xb):
    """control points [4][c] of the cubics through nodes4 [4][c] (at XI in the segment's coordinate) restricted to [xa, xb] of that coordinate, and
    their values [c] at the middle of it.  Power basis: the segment's cubic, then its Taylor coefficients at xa scaled to u in [0, 1]"""
    nodes4 = np.asarray(nodes4, float).reshape(4, -1)
    power = np.linalg.solve(np.vander(XI, 4, increasing=True), nodes4)            # [4][c], the segment's cubics
    dx = xb - xa
    coef = np.stack([P.polyval(xa, P.polyder(power, k)) * dx ** k / [1.0, 1.0, 2.0, 6.0][k] if k else P.polyval(xa, power) for k in range(4)])
    return POWER_TO_BERNSTEIN @ coef, P.polyval(0.5, coef)


def certified_np(models, tables, obstacles, nseg, x, T, margin, self_gap, n_start, max_depth):
    """models: [(R0, p)] per arm; tables: one sphere record array per arm; obstacles: records or None; x [N][14 narm]"""
    narm, nq = len(models), 7 * len(models)
    q = np.asarray(x, float)[:, :nq]
    n0 = nseg * n_start
    assert 1 <= n0 <= CAPACITY and 0 <= max_depth <= 16
    if not np.isfinite(q).all():
        return dict(clr=dict(d_min=np.nan, t_min=-1.0, t_first=-1.0, sphere=-1, other=0, n_hit=0, status=NAN),
                    cert=dict(d_lower=np.nan, t_lower=-1.0, n_eval=0, n_clear=0, n_undecided=0, depth=0), gap=np.inf)
    arm = [a for a in range(narm) for _ in range(len(tables[a]))]
    sph = [s for a in range(narm) for s in tables[a]]
    jnt = [int(s["joint"]) for s in sph]
    cs = np.array([s["c"] for s in sph], float).reshape(-1, 3)
    rad = np.array([s["r"] for s in sph], float)
    nsph = len(sph)
    obs = [] if obstacles is None else list(obstacles)
    reach = np.zeros((nsph, 7))
    for s in range(nsph):
        plen = np.linalg.norm(models[arm[s]][1], axis=1)
        for i in range(jnt[s] + 1):
            reach[s, i] = np.linalg.norm(cs[s]) + plen[i + 1:jnt[s] + 1].sum()
    robot_pairs = [(s, t) for s in range(nsph) for t in range(s + 1, nsph)
                   if arm[s] != arm[t] or (self_gap > 0 and abs(jnt[s] - jnt[t]) >= self_gap)]
    ps_, pt_ = np.array([p[0] for p in robot_pairs], int), np.array([p[1] for p in robot_pairs], int)

    best = (np.inf, None)               # (d, (t_m, sphere, robot, index))
    lower = (np.inf, None)              # (L, t_m)
    hits, n_clear, n_und, n_eval, depth, gap = [], 0, 0, 0, 0, np.inf
    level = list(range(n0))
    l = 0
    while level:
        depth = l
        den = n0 * 2 ** l
        nxt, n_split = [], 0
        for i in level:
            tm = Fraction(2 * i + 1, 2 * den)
            seg = i // (n_start * 2 ** l)
            xa, xb = 2.0 * (i / den * nseg - seg) - 1.0, 2.0 * ((i + 1) / den * nseg - seg) - 1.0
            ctrl, qm = bezier_of_interval(q[3 * seg:3 * seg + 4], xa, xb)
            dev = np.abs(ctrl - qm[None]).max(axis=0)
            cen = np.zeros((nsph, 3))
            for a in range(narm):
                Rs, ps = frames(models[a], qm[7 * a:7 * a + 7])
                for s in range(nsph):
                    if arm[s] == a:
                        cen[s] = ps[jnt[s]] + Rs[jnt[s]] @ cs[s]
            D = np.array([reach[s] @ dev[7 * arm[s]:7 * arm[s] + 7] for s in range(nsph)])
            d_mid, L = np.inf, np.inf
            cand = []
            if obs and nsph:
                dob = np.stack([signed_distance(ob, cen) for ob in obs], axis=1) - rad[:, None]          # [nsph][n_obs]
                d_mid, L = min(d_mid, dob.min()), min(L, (dob - D[:, None]).min())
                s, o = np.unravel_index(np.argmin(dob), dob.shape)          # (row-major: the lowest sphere, then the lowest obstacle)
                cand.append((dob[s, o], (tm, int(s), 0, int(o))))
            if robot_pairs:
                drb = np.linalg.norm(cen[ps_] - cen[pt_], axis=1) - rad[ps_] - rad[pt_]
                d_mid, L = min(d_mid, drb.min()), min(L, (drb - D[ps_] - D[pt_]).min())
                k = int(np.argmin(drb))                                     # (the pair list is ordered by s, then t)
                cand.append((drb[k], (tm, int(ps_[k]), 1, int(pt_[k]))))
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
                    nxt += [2 * i, 2 * i + 1]
                    continue
                else:
                    what = "undecided"
            if what == "hit":
                hits.append(tm)
            elif what == "clear":
                n_clear += 1
            else:
                n_und += 1
            if L < lower[0] or (L == lower[0] and (lower[1] is None or tm < lower[1])):
                lower = (L, tm)
        level = nxt
        l += 1
    clr = dict(d_min=best[0], n_hit=len(hits), t_first=float(min(hits)) * T if hits else -1.0,
               status=(HIT if hits else 0) | (UNDECIDED if n_und else 0))
    if best[1] is None:
        clr.update(t_min=-1.0, sphere=-1, other=0)
    else:
        tm, s, robot, idx = best[1]
        clr.update(t_min=float(tm) * T, sphere=s, other=-1 - idx if robot else idx)
    cert = dict(d_lower=lower[0], t_lower=float(lower[1]) * T, n_eval=n_eval, n_clear=n_clear, n_undecided=n_und, depth=depth)
    return dict(clr=clr, cert=cert, gap=gap)
