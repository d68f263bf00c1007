"""The rule of include/mpcmp_retimed_check.h in NumPy, composed of the references the suite already has; independent of csrc/.

A retimed plan is sampled by retime_reference.sample_retimed_np and a retimed route by route_retime_reference.sample_retimed_route_np (the rows of
mpcmp_sample_retimed_batch / mpcmp_sample_retimed_route_batch: the time, then per arm q, qd, qdd, tau).  The tool height and the tool speeds of those
rows come from test_limits_host.values_np, and the record from test_limits_host.record_np: for a plan at once, for a route from the excesses and
ratios of every leg's samples under that leg's row (groups_np, ratios_np), put together by the lines record_np ends with.  What is written here is
only what the header adds: which leg a sample of the route clock belongs to, the time base T_new, and the record of a failed profile.
tests/test_retimed_check_host.py checks mpcmp_limits_retimed_one against it and tests/test_gpu_retimed_check.py the kernels.
"""
import numpy as np

import retime_reference as R
import route_retime_reference as RR
from test_limits_host import GROUPS, groups_np, ratios_np, record_np, values_np

NAN = 128


def failed_record():
    """the record of a profile whose t_n is not finite"""
    return dict(failed=True, status=NAN, excess=np.full(GROUPS, np.nan), n_viol=0, t_first=-1.0, stretch=1.0, T_new=np.inf, near=False)


def _values(models, rows):
    """sampler rows [S][1 + 28 narm] -> the dict of values_np (the sampler's torque kept)"""
    narm = len(models)
    cat = lambda lo: np.concatenate([rows[:, 1 + 28 * a + lo:8 + 28 * a + lo] for a in range(narm)], axis=1)
    return values_np(models, cat(0), cat(7), cat(14), tau=cat(21))


def plan_record_np(models, nseg, sx, su, T, prof, row, n_pts, tol, lin_max=np.inf, ang_max=np.inf):
    """one plan sx [N][14 narm], su [N][7 narm], T under prof [n + 1][2] and the bounds record row -> the dict of record_np with T_new and the sampled
    values under "v"; times are those of the retimed clock"""
    T_new = prof[-1, 0]
    if not np.isfinite(T_new):
        return failed_record()
    v = _values(models, R.sample_retimed_np(models, nseg, sx, su, T, prof, n_pts))
    r = record_np(v, row, T_new, n_pts, tol, lin_max, ang_max)
    r.update(failed=False, T_new=T_new, v=v)
    return r


def route_legs_np(prof, n_pts):
    """the leg of every sample of the route clock, by the rule of mpcmp_sample_retimed_route_batch: prof [M+1][n + 1][2] -> (legs [n_pts + 1], T_new)"""
    nl, D = prof.shape[0], prof[:, -1, 0]
    T_new = D[0]
    for m in range(1, nl):
        T_new = T_new + D[m]
    legs = np.zeros(n_pts + 1, dtype=int)
    for i in range(n_pts + 1):
        t = (i / n_pts) * T_new
        Ep, m = 0.0, 0
        while True:
            E = Ep + D[m]
            if t < E or m == nl - 1:
                break
            Ep, m = E, m + 1
        legs[i] = nl - 1 if i == n_pts else m
    return legs, T_new


def route_record_np(models, nseg, sx, su, sT, prof, rows, n_pts, tol, lin_max=np.inf, ang_max=np.inf):
    """one route sx [M+1][N][14 narm], su, sT [M+1] under prof [M+1][n + 1][2] and the bounds records rows [M+1] -> the dict of record_np; models: one
    list, or one per leg (payload rows)"""
    if not np.isfinite(prof[:, -1, 0]).all():
        return failed_record()
    legs, T_new = route_legs_np(prof, n_pts)
    samples = RR.sample_retimed_route_np(models, nseg, sx, su, sT, prof, n_pts)
    per_leg = isinstance(models[0], (list, tuple))
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (GROUPS,))
    E, ratios = None, np.zeros(4)
    for m in np.unique(legs):
        idx = np.flatnonzero(legs == m)
        v = _values(models[m] if per_leg else models, samples[idx])
        Em = groups_np(v, rows[m], lin_max, ang_max)
        if E is None:
            E = [np.full((n_pts + 1,) + e.shape[1:], -np.inf) for e in Em]
        for e, em in zip(E, Em):
            e[idx] = em
        ratios = np.maximum(ratios, ratios_np(v, rows[m], lin_max, ang_max))
    # the lines record_np ends with
    per_sample = np.stack([e.max(axis=1) for e in E], axis=1)
    excess = per_sample.max(axis=0)
    over = (per_sample > tol).any(axis=1)
    first = int(np.argmax(over)) if over.any() else -1
    return dict(E=E, per_sample=per_sample, excess=excess, status=sum(1 << g for g in range(GROUPS) if excess[g] > tol[g]), n_viol=int(over.sum()),
                t_first=(first / n_pts) * T_new if first >= 0 else -1.0, ratios=ratios, stretch=max(1.0, ratios[0], np.sqrt(ratios[1]), ratios[2], ratios[3]),
                near=bool((np.abs(per_sample - tol) <= 1e-8).any()), failed=False, T_new=T_new, legs=legs)


def scale_np(prof, f):
    """the scale rule: t_k *= f, x_k /= f^2; a factor that is not finite or <= 0 gives a NaN profile"""
    out = np.array(prof, dtype=np.float64)
    if not (np.isfinite(f) and f > 0):
        out[:] = np.nan
        return out
    out[..., 0] = out[..., 0] * f
    out[..., 1] = out[..., 1] / (f * f)
    return out
