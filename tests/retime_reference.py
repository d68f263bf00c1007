"""The retiming rule of include/mpcmp_retime.h in NumPy, written from the header text; independent of csrc/retime.hpp.

Per arm q, v, a and RNEA(q, v, a) at the grid points come from oracle_py.sample, c = RNEA(q, 0, 0) and RNEA(q, 0, v) from oracle_py.rnea, the tool
speeds from oracle_py.frame_jacobian at the tool point (a norm does not care which frame the Jacobian is expressed in).  The elimination of w over the
(row with A > 0, row with A < 0) pairs of a grid point is one outer product per grid point.  tests/test_retime_host.py checks mpcmp_retime_one
against it and tests/test_gpu_retime.py the kernels.
"""
import numpy as np

import oracle_py as o

QD, QDD, TAU, TOOL_LIN, TOOL_ANG = 1, 2, 3, 5, 6
ALL_GROUPS = (1 << QD) | (1 << QDD) | (1 << TAU) | (1 << TOOL_LIN) | (1 << TOOL_ANG)
INFEASIBLE, NAN = 1, 128
ZERO_A = 1e-12
XI = np.array([-1.0, -0.5, 0.5, 1.0])


def omodel(m):
    return o.Model.from_buffer_copy(m)


def arm_nodes(sx, su, a):
    """the nodes of arm a of one trajectory sx [N][14 narm], su [N][7 narm] as a one-arm trajectory [N][14], [N][7]"""
    nq = sx.shape[1] // 2
    return np.concatenate([sx[:, 7 * a:7 * a + 7], sx[:, nq + 7 * a:nq + 7 * a + 7]], axis=1), su[:, 7 * a:7 * a + 7]


def path_values(models, nseg, sx, su, T, n_grid, scale=None):
    """what the rows are made of, at the n_grid + 1 grid points: q, v, a, c, d1, d2 [n + 1][7 narm], vlin, vang [n + 1][narm].
    scale (q, v, a) [n + 1][7 narm] each, or None: factors on the sampled q, v, a before anything is formed from them (a perturbation run)"""
    narm, S = len(models), n_grid + 1
    P = {k: np.zeros((S, 7 * narm)) for k in ("q", "v", "a", "c", "d1", "d2")}
    P["vlin"], P["vang"] = np.zeros((S, narm)), np.zeros((S, narm))
    z = np.zeros(7)
    for a, m in enumerate(models):
        om, tool, cs = omodel(m), np.array(m.tool[:]), slice(7 * a, 7 * a + 7)
        xa, ua = arm_nodes(sx, su, a)
        rows = o.sample(nseg, xa, ua, T, n_grid, model=om)
        P["q"][:, cs], P["v"][:, cs], P["a"][:, cs] = rows[:, 1:8], rows[:, 8:15], rows[:, 15:22]
        if scale is not None:
            for name, f in zip(("q", "v", "a"), scale):
                P[name][:, cs] *= f[:, cs]
        for k in range(S):
            q, v = P["q"][k, cs], P["v"][k, cs]
            c = o.rnea(q, z, z, model=om)
            P["c"][k, cs] = c
            P["d1"][k, cs] = (rows[k, 22:29] if scale is None else o.rnea(q, v, P["a"][k, cs], model=om)) - c
            P["d2"][k, cs] = o.rnea(q, z, v, model=om) - c
            tw = o.frame_jacobian(q, tool, model=om) @ v
            P["vlin"][k, a], P["vang"][k, a] = np.linalg.norm(tw[:3]), np.linalg.norm(tw[3:])
    return P


def _speed_cap(v, lb, ub):
    """x <= (bound / v)^2 with the bound on v's side; +inf for v == 0 or an infinite bound, 0 for a bound no slowing down meets"""
    cap = np.full(v.shape, np.inf)
    lb, ub = np.broadcast_to(lb, v.shape), np.broadcast_to(ub, v.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pos, neg = v > 0, v < 0
        cap[pos] = np.where(np.isposinf(ub[pos]), np.inf, np.where(ub[pos] <= 0, 0.0, (ub[pos] / v[pos]) ** 2))
        cap[neg] = np.where(np.isneginf(lb[neg]), np.inf, np.where(lb[neg] >= 0, 0.0, (lb[neg] / v[neg]) ** 2))
    return cap


def caps_np(P, row, lin_max, ang_max, rate_max, groups):
    """cap_k [n + 1] without the rows whose A is 0"""
    narm = P["vlin"].shape[1]
    cap = np.full(P["v"].shape[0], rate_max * rate_max)
    if groups >> QD & 1:
        cap = np.minimum(cap, _speed_cap(P["v"], np.tile(row["lbx"][7:], narm), np.tile(row["ubx"][7:], narm)).min(axis=1))
    if groups >> TOOL_LIN & 1:
        cap = np.minimum(cap, _speed_cap(P["vlin"], -np.inf, lin_max).min(axis=1))
    if groups >> TOOL_ANG & 1:
        cap = np.minimum(cap, _speed_cap(P["vang"], -np.inf, ang_max).min(axis=1))
    return cap


def rows_np(P, row, T, groups):
    """A, B, C [n + 1][R]: the QDD and TAU rows A w + B x + C <= 0 of every grid point; a row that is not there is (0, 0, -1)"""
    narm = P["vlin"].shape[1]
    h = 1.0 / (2.0 * T)
    t = lambda name: np.tile(np.asarray(row[name], dtype=np.float64)[:7], narm)
    parts = []
    zero = np.zeros_like(P["c"])
    for g, a, b, c, lb, ub in ((QDD, P["v"] * h, P["a"], zero, t("lbu"), t("ubu")), (TAU, P["d2"] * h, P["d1"], P["c"], t("lbg"), t("ubg"))):
        for A, B, C, bound in ((a, b, c - ub, ub), (-a, -b, lb - c, lb)):
            off = ~np.isfinite(bound) if groups >> g & 1 else np.ones(bound.shape, dtype=bool)
            off = np.broadcast_to(off, A.shape)
            with np.errstate(invalid="ignore"):
                A, B, C = np.where(off, 0.0, A), np.where(off, 0.0, B), np.where(off, -1.0, C)
            parts.append((A, B, C))
    A, B, C = [np.concatenate([p[i] for p in parts], axis=1) for i in range(3)]
    A = np.where(np.abs(A) <= ZERO_A * (np.abs(B) + np.abs(C) + 1.0), 0.0, A)
    return A, B, C


def _cut(lo, hi, empty, Bx, Cx):
    """the rows Bx x + Cx <= 0 (any shape) applied to [lo, hi]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = -Cx / Bx
    if (Bx > 0).any():
        hi = min(hi, r[Bx > 0].min())
    if (Bx < 0).any():
        lo = max(lo, r[Bx < 0].max())
    return lo, hi, empty or bool(((Bx == 0) & (Cx > 0)).any())


def retime_np(P, row, T, n_grid, lin_max=np.inf, ang_max=np.inf, rate_max=1.0, groups=ALL_GROUPS):
    """-> dict: status, k_fail, T_new, rate_min, s_slowest, n_slowed, t [n + 1], x [n + 1], lo, hi [n + 1], A, B, C, cap, and
    `near`: some controllable set within 1e-8 (relative) of empty, or of not being empty where the plan is reported infeasible"""
    n, delta = n_grid, 1.0 / n_grid
    A, B, C = rows_np(P, row, T, groups)
    cap = caps_np(P, row, lin_max, ang_max, rate_max, groups)
    pin0, pinn = bool((P["v"][0] != 0).any()), bool((P["v"][n] != 0).any())
    lo, hi = np.zeros(n + 1), np.zeros(n + 1)
    out = dict(A=A, B=B, C=C, cap=cap, lo=lo, hi=hi, status=0, k_fail=-1, T_new=np.inf, rate_min=0.0, s_slowest=-1.0, n_slowed=0,
               t=np.full(n + 1, np.nan), x=np.full(n + 1, np.nan), near=False, pin0=pin0, pinn=pinn)
    for k in range(n, -1, -1):
        a, b, c = A[k], B[k], C[k]
        if k < n:
            a, b, c = np.append(a, [delta, -delta]), np.append(b, [1.0, -1.0]), np.append(c, [-hi[k + 1], lo[k + 1]])
        l, h, empty = _cut(0.0, cap[k], False, b[a == 0], c[a == 0])
        if k < n:
            up, dn = a > 0, a < 0
            Pm = np.outer(a[up], b[dn]) - np.outer(b[up], a[dn])
            Qm = np.outer(a[up], c[dn]) - np.outer(c[up], a[dn])
            l, h, empty = _cut(l, h, empty, Pm, Qm)
        fail = empty or not l <= h or h == 0.0
        pinned = (k == n and pinn) or (k == 0 and pin0)
        if pinned:
            fail = fail or not (l <= 1.0 <= h)
            out["near"] |= abs(l - 1.0) <= 1e-8 or abs(h - 1.0) <= 1e-8
        else:
            out["near"] |= bool(abs(h - l) <= 1e-8 * max(abs(h), abs(l)) or 0.0 < h <= 1e-8)
        if fail:
            out.update(status=INFEASIBLE, k_fail=k)
            return out
        if k == n and pinn:
            l = h = 1.0
        lo[k], hi[k] = l, h
    x, t = out["x"], out["t"]
    x[0], t[0] = (1.0 if pin0 else hi[0]), 0.0
    for k in range(n):
        a, b, c = np.append(A[k], delta), np.append(B[k], 1.0), np.append(C[k], -hi[k + 1])
        up = a > 0
        w = (-(b[up] * x[k] + c[up]) / a[up]).min()
        x[k + 1] = min(max(x[k] + delta * w, lo[k + 1]), hi[k + 1])
        with np.errstate(divide="ignore"):
            t[k + 1] = t[k] + 2.0 * T * delta / (np.sqrt(x[k]) + np.sqrt(x[k + 1]))
    if not np.isfinite(t[n]):
        x[:], t[:] = np.nan, np.nan
        out.update(status=INFEASIBLE, k_fail=-1)
        return out
    kmin = int(np.argmin(x))
    out.update(T_new=t[n], rate_min=float(np.sqrt(x[kmin])), s_slowest=kmin / n, n_slowed=int((x < rate_max * rate_max).sum()))
    return out


def motion_np(P, T, x):
    """the retimed motion at the grid points from a profile x [n + 1], with the interval's w (at the last point that of the interval before it):
    qd, qdd, tau [n + 1][7 narm], vlin, vang [n + 1][narm]"""
    n = x.shape[0] - 1
    w = np.diff(x) * n
    w = np.append(w, w[-1])[:, None]
    lam, xx, h = np.sqrt(x)[:, None], x[:, None], 1.0 / (2.0 * T)
    return dict(qd=lam * P["v"], qdd=xx * P["a"] + w * h * P["v"], tau=P["c"] + xx * P["d1"] + w * h * P["d2"], vlin=lam * P["vlin"], vang=lam * P["vang"])


def lagrange_np(nseg, nodes, s):
    """the Lagrange rule of mpcmp_sample_batch: nodes [N][c] at the normalised time s -> [c]"""
    seg = min(max(int(np.floor(s * nseg)), 0), nseg - 1)
    xx = 2.0 * (s * nseg - seg) - 1.0
    L = np.array([np.prod([(xx - XI[k]) / (XI[j] - XI[k]) for k in range(4) if k != j]) for j in range(4)])
    return L @ nodes[3 * seg:3 * seg + 4]


def sample_retimed_np(models, nseg, sx, su, T, prof, n_pts):
    """the retimed-sample rule: [n_pts + 1][1 + 28 narm]"""
    narm, n = len(models), prof.shape[0] - 1
    out = np.full((n_pts + 1, 1 + 28 * narm), np.nan)
    t_k, x_k = prof[:, 0], prof[:, 1]
    if not np.isfinite(t_k[n]):
        return out
    h = 1.0 / (2.0 * T)
    for i in range(n_pts + 1):
        t = (i / n_pts) * t_k[n]
        k = min(max(int(np.searchsorted(t_k, t, side="right")) - 1, 0), n - 1)
        lk, w = np.sqrt(x_k[k]), (x_k[k + 1] - x_k[k]) * n
        lam = lk + w * (t - t_k[k]) * h
        s = k / n + (t - t_k[k]) * (lk + lam) * h
        if i == n_pts:
            lam, s = np.sqrt(x_k[n]), 1.0
        s = min(max(s, 0.0), 1.0)
        out[i, 0] = t
        for a, m in enumerate(models):
            xa, ua = arm_nodes(sx, su, a)
            q, v, ac = lagrange_np(nseg, xa[:, :7], s), lagrange_np(nseg, xa[:, 7:], s), lagrange_np(nseg, ua, s)
            qd, qdd = lam * v, lam * lam * ac + w * h * v
            out[i, 1 + 28 * a:29 + 28 * a] = np.concatenate([q, qd, qdd, o.rnea(q, qd, qdd, model=omodel(m))])
    return out
