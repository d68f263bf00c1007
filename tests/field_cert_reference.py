"""NumPy restatement of the certified clearance rule against a voxel world (include/mpcmp_field_cert.h) that shares nothing with the library.  It
composes what the suite already has: bezier_of_interval and frames of tests/clearance_cert_reference.py with exact rational midpoints, and sd_field
and face_distance of tests/field_reference.py.  Only the level loop and the per-sphere distances are written here, from the header text.

certified_field_np returns the two records as dicts plus
  gap   its smallest decision gap, as certified_np defines it: the minimum over all decisions it took of |d_mid - margin| and |L - margin|;
  face  the smallest distance of any evaluated sphere centre to an interior voxel face, where sd_field jumps.
A test compares integer fields only where both are far above the rounding of either side.  merge_cert is the certificate merge in a few lines.
"""
from fractions import Fraction

import numpy as np

import clearance_cert_reference as R
import field_reference as F

HIT, NAN, UNDECIDED = R.HIT, R.NAN, R.UNDECIDED
CERT_DTYPE = np.dtype([("d_lower", "f8"), ("t_lower", "f8"), ("n_eval", "i4"), ("n_clear", "i4"), ("n_undecided", "i4"), ("depth", "i4")])


def certified_field_np(models, tables, origin, h, n, d2, nseg, x, T, margin, n_start, max_depth):
    """models: [(R0, p)] per arm; tables: one sphere record array per arm; the grid (origin, h, n = (n0, n1, n2)) with its field d2; x [N][14 narm]"""
    narm, nq = len(models), 7 * len(models)
    q = np.asarray(x, float)[:, :nq]
    n0 = nseg * n_start
    assert 1 <= n0 <= R.CAPACITY and 0 <= max_depth <= 16
    if not np.isfinite(q).all():
        return dict(clr=dict(d_min=np.nan, t_min=-1.0, t_first=-1.0, sphere=-1, other=0, n_hit=0, status=NAN),
                    cert=dict(d_lower=np.nan, t_lower=-1.0, n_eval=0, n_clear=0, n_undecided=0, depth=0), gap=np.inf, face=np.inf)
    arm = [a for a in range(narm) for _ in range(len(tables[a]))]
    sph = [s for a in range(narm) for s in tables[a]]
    jnt = [int(s["joint"]) for s in sph]
    cs = np.array([s["c"] for s in sph], float).reshape(-1, 3)
    rad = np.array([s["r"] for s in sph], float)
    nsph = len(sph)
    reach = np.zeros((nsph, 7))
    for s in range(nsph):
        plen = np.linalg.norm(models[arm[s]][1], axis=1)
        for i in range(jnt[s] + 1):
            reach[s, i] = np.linalg.norm(cs[s]) + plen[i + 1:jnt[s] + 1].sum()

    best = (np.inf, None, 0)            # (d, (t_m, sphere), voxel)
    lower = (np.inf, None)              # (L, t_m)
    hits, n_clear, n_und, n_eval, depth, gap, face = [], 0, 0, 0, 0, np.inf, np.inf
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
            ctrl, qm = R.bezier_of_interval(q[3 * seg:3 * seg + 4], xa, xb)
            dev = np.abs(ctrl - qm[None]).max(axis=0)
            d_mid, L = np.inf, np.inf
            if nsph:
                cen = np.zeros((nsph, 3))
                for a in range(narm):
                    Rs, ps = R.frames(models[a], qm[7 * a:7 * a + 7])
                    for s in range(nsph):
                        if arm[s] == a:
                            cen[s] = ps[jnt[s]] + Rs[jnt[s]] @ cs[s]
                D = np.array([reach[s] @ dev[7 * arm[s]:7 * arm[s] + 7] for s in range(nsph)])
                sd, vox = F.sd_field(origin, h, n, d2, cen)
                d = sd - rad
                face = min(face, float(F.face_distance(origin, h, n, cen).min()))
                d_mid, L = d.min(), (d - D).min()
                s = int(np.argmin(d))                                           # (the lowest sphere among equals)
                if np.isfinite(d[s]) and (d[s] < best[0] or (d[s] == best[0] and (tm, s) < best[1])):
                    best = (d[s], (tm, s), int(vox[s]))
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
                elif n_split < R.SPLIT_MAX:
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
        clr.update(t_min=float(best[1][0]) * T, sphere=best[1][1], other=best[2])
    cert = dict(d_lower=lower[0], t_lower=float(lower[1]) * T, n_eval=n_eval, n_clear=n_clear, n_undecided=n_und, depth=depth)
    return dict(clr=clr, cert=cert, gap=gap, face=face)


def merge_cert(a, b):
    """the rule of mpcmp_clearance_cert_merge_batch on two certificate arrays"""
    out = np.zeros(a.shape[0], dtype=a.dtype)
    for i in range(a.shape[0]):
        if np.isnan(a[i]["d_lower"]) or np.isnan(b[i]["d_lower"]):
            out[i] = (np.nan, -1.0, 0, 0, 0, 0)
            continue
        w = b[i] if b[i]["d_lower"] < a[i]["d_lower"] else a[i]
        out[i] = (w["d_lower"], w["t_lower"], a[i]["n_eval"] + b[i]["n_eval"], a[i]["n_clear"] + b[i]["n_clear"],
                  a[i]["n_undecided"] + b[i]["n_undecided"], max(a[i]["depth"], b[i]["depth"]))
    return out
