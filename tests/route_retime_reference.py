"""The route retiming rule of include/mpcmp_route_retime.h in NumPy, written from the header text; independent of csrc/.

A route is a list of legs.  Per leg the path values of the grid points, the rows, the caps and the cut of an interval by rows are those of
tests/retime_reference.py (the header says: everything follows mpcmp_retime.h except what it lists); what is written here is what the header lists:
the grid per leg, the junction sets of the backward pass, the carried x of the forward pass, the clock per leg, the record of a route and the
sampler on one clock.  tests/test_route_retime_host.py checks mpcmp_retime_route_one against it and tests/test_gpu_route_retime.py the kernels.
"""
import numpy as np

import retime_reference as R

INFEASIBLE, NAN = R.INFEASIBLE, R.NAN


def route_path_values(models, nseg, sx, su, sT, n_grid, scale=None):
    """per leg the dict of retime_reference.path_values; sx [M+1][N][14 narm], su, sT [M+1]; scale: None or one (q, v, a) triple per leg"""
    return [R.path_values(models, nseg, sx[m], su[m], sT[m], n_grid, None if scale is None else scale[m]) for m in range(sT.shape[0])]


def retime_route_np(P, rows, T, n_grid, lin_max=np.inf, ang_max=np.inf, rate_max=1.0, groups=R.ALL_GROUPS):
    """P, rows, T: per leg.  -> dict: status, leg_fail, k_fail, T_new, leg_T_new [M+1], rate_min, s_slowest, leg_slowest, n_slowed, t, x, lo, hi
    [M+1][n + 1], and `near`: some set within 1e-8 (relative) of empty, or of not being empty where the route is reported infeasible"""
    n, delta, nl = n_grid, 1.0 / n_grid, len(P)
    rows_of = [R.rows_np(P[m], rows[m], T[m], groups) for m in range(nl)]
    cap = [R.caps_np(P[m], rows[m], lin_max, ang_max, rate_max, groups) for m in range(nl)]
    pin0, pinn = bool((P[0]["v"][0] != 0).any()), bool((P[nl - 1]["v"][n] != 0).any())
    lo, hi = np.zeros((nl, n + 1)), np.zeros((nl, n + 1))
    out = dict(lo=lo, hi=hi, status=0, leg_fail=-1, k_fail=-1, T_new=np.inf, leg_T_new=np.full(nl, np.inf), rate_min=0.0, s_slowest=-1.0,
               leg_slowest=-1, n_slowed=0, t=np.full((nl, n + 1), np.nan), x=np.full((nl, n + 1), np.nan), near=False, pin0=pin0, pinn=pinn)
    for m in range(nl - 1, -1, -1):
        A, B, C = rows_of[m]
        for k in range(n, -1, -1):
            a, b, c = A[k], B[k], C[k]
            if k < n:
                a, b, c = np.append(a, [delta, -delta]), np.append(b, [1.0, -1.0]), np.append(c, [-hi[m, k + 1], lo[m, k + 1]])
            l, h, empty = R._cut(0.0, cap[m][k], False, b[a == 0], c[a == 0])
            if k < n:
                up, dn = a > 0, a < 0
                l, h, empty = R._cut(l, h, empty, np.outer(a[up], b[dn]) - np.outer(b[up], a[dn]), np.outer(a[up], c[dn]) - np.outer(c[up], a[dn]))
            elif m < nl - 1:                      # a junction: within K_0 of the later leg
                l, h = max(l, lo[m + 1, 0]), min(h, hi[m + 1, 0])
            fail = empty or not l <= h or h == 0.0
            pinned = (k == n and m == nl - 1 and pinn) or (k == 0 and m == 0 and pin0)
            if pinned:
                fail = fail or not (l <= 1.0 <= h)
                out["near"] |= abs(l - 1.0) <= 1e-8 or abs(h - 1.0) <= 1e-8
            else:
                out["near"] |= bool(abs(h - l) <= 1e-8 * max(abs(h), abs(l)) or 0.0 < h <= 1e-8)
            if fail:
                out.update(status=INFEASIBLE, leg_fail=m, k_fail=k)
                return out
            if pinned and k == n:
                l = h = 1.0
            lo[m, k], hi[m, k] = l, h
    x, t = out["x"], out["t"]
    xk, T_new = (1.0 if pin0 else hi[0, 0]), 0.0
    for m in range(nl):
        A, B, C = rows_of[m]
        x[m, 0], t[m, 0] = xk, 0.0
        for k in range(n):
            a, b, c = np.append(A[k], delta), np.append(B[k], 1.0), np.append(C[k], -hi[m, k + 1])
            up = a > 0
            w = (-(b[up] * x[m, k] + c[up]) / a[up]).min()
            x[m, k + 1] = min(max(x[m, k] + delta * w, lo[m, k + 1]), hi[m, k + 1])
            with np.errstate(divide="ignore"):
                t[m, k + 1] = t[m, k] + 2.0 * T[m] * delta / (np.sqrt(x[m, k]) + np.sqrt(x[m, k + 1]))
        xk = x[m, n]
        T_new = t[m, n] if m == 0 else T_new + t[m, n]
    if not np.isfinite(T_new):
        x[:], t[:] = np.nan, np.nan
        out.update(status=INFEASIBLE)
        return out
    flat = int(np.argmin(x))                      # the first minimum in route order: the lowest leg, then the lowest k
    lm, km = divmod(flat, n + 1)
    slowed = x < rate_max * rate_max
    out.update(T_new=T_new, leg_T_new=t[:, n].copy(), rate_min=float(np.sqrt(x[lm, km])), s_slowest=km / n, leg_slowest=lm,
               n_slowed=int(slowed[0].sum() + slowed[1:, 1:].sum()))
    return out


def sample_retimed_route_np(models, nseg, sx, su, sT, prof, n_pts):
    """the sampler of a retimed route: sx [M+1][N][14 narm], prof [M+1][n + 1][2] -> [n_pts + 1][1 + 28 narm]; models: one list, or one per leg"""
    nl, n = prof.shape[0], prof.shape[1] - 1
    narm = sx.shape[2] // 14
    out = np.full((n_pts + 1, 1 + 28 * narm), np.nan)
    D = prof[:, n, 0]
    if not np.isfinite(D).all():
        return out
    T_new = D[0]
    for m in range(1, nl):
        T_new = T_new + D[m]
    for i in range(n_pts + 1):
        t = (i / n_pts) * T_new
        Ep, m = 0.0, 0
        while True:
            E = Ep + D[m]
            if t < E or m == nl - 1:
                break
            Ep, m = E, m + 1
        if i == n_pts:
            m = nl - 1
        tl = min(max(t - Ep, 0.0), D[m])
        t_k, x_k, h = prof[m, :, 0], prof[m, :, 1], 1.0 / (2.0 * sT[m])
        k = min(max(int(np.searchsorted(t_k, tl, side="right")) - 1, 0), n - 1)
        if i == n_pts:
            k = n - 1
        lk, w = np.sqrt(x_k[k]), (x_k[k + 1] - x_k[k]) * n
        lam = lk + w * (tl - t_k[k]) * h
        s = k / n + (tl - t_k[k]) * (lk + lam) * h
        if i == n_pts:
            lam, s = np.sqrt(x_k[n]), 1.0
        s = min(max(s, 0.0), 1.0)
        out[i, 0] = t
        mm = models[m] if isinstance(models[0], (list, tuple)) else models
        for a, mdl in enumerate(mm):
            xa, ua = R.arm_nodes(sx[m], su[m], a)
            q, v, ac = R.lagrange_np(nseg, xa[:, :7], s), R.lagrange_np(nseg, xa[:, 7:], s), R.lagrange_np(nseg, ua, s)
            qd, qdd = lam * v, lam * lam * ac + w * h * v
            out[i, 1 + 28 * a:29 + 28 * a] = np.concatenate([q, qd, qdd, R.o.rnea(q, qd, qdd, model=R.omodel(mdl))])
    return out
