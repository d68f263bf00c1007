"""NumPy / SciPy reference of the voxel worlds (include/mpcmp_field.h).  It shares nothing with the library: the transform is SciPy's exact Euclidean
distance transform, squared and rounded (itself pinned to a brute-force minimum on tiny grids by tests/test_field_host.py), the distance of a point
and the clearance record are written out from the header's rule on the forward kinematics of tests/test_clearance_host.py and the samples of
oracle_py.sample, and the true distance to the occupied cubes is a brute-force minimum over them.

Arrays are indexed [k][j][i] = [z][y][x]; the linear index of voxel (i, j, k) is (k n1 + j) n0 + i, that of a C-ordered array."""
import numpy as np
from scipy import ndimage

import oracle_py as o
from test_clearance_host import sd_np, sphere_centres

EMPTY = 0xFFFFFFFF
HALF_DIAGONAL = np.sqrt(3.0) / 2.0


def edt_brute(occ):
    """d2 [n2][n1][n0]: min over occupied w of |v - w|^2, by comparing every voxel with every occupied one"""
    occ = np.asarray(occ) != 0
    w = np.argwhere(occ)
    if w.shape[0] == 0:
        return np.full(occ.shape, EMPTY, dtype=np.uint32)
    v = np.argwhere(np.ones(occ.shape, dtype=bool))
    d = ((v[:, None, :] - w[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return d.reshape(occ.shape).astype(np.uint32)


def edt(occ):
    """the same by scipy.ndimage.distance_transform_edt (exact), squared and rounded to the integer it is"""
    occ = np.asarray(occ) != 0
    if not occ.any():
        return np.full(occ.shape, EMPTY, dtype=np.uint32)
    return np.rint(ndimage.distance_transform_edt(~occ) ** 2).astype(np.uint32)


def mark_points(origin, h, n, points):
    """occupancy [n2][n1][n0] of the voxels that contain a point; non-finite points and points outside 0 <= u < n are skipped"""
    occ = np.zeros((n[2], n[1], n[0]), dtype=np.uint8)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        u = (p - np.asarray(origin)) / h
        ok = np.isfinite(p).all(axis=1) & (u >= 0).all(axis=1) & (u < np.asarray(n)).all(axis=1)
    v = np.floor(u[ok]).astype(int)
    occ[v[:, 2], v[:, 1], v[:, 0]] = 1
    return occ


def face_distance(origin, h, n, x):
    """world distance of the points x [..., 3] to the nearest INTERIOR voxel face (a plane u_d = 1 .. n_d - 1 with u inside the grid's range on
    that axis): where sd_field jumps.  inf where an axis has no interior face near the point's clamped position"""
    u = (np.asarray(x, dtype=np.float64) - np.asarray(origin)) / h
    n = np.asarray(n)
    r = np.rint(u)
    d = np.abs(u - r)
    d = np.where((r >= 1) & (r <= n - 1), d, np.inf)
    return h * d.min(axis=-1)


def sd_field(origin, h, n, d2, x):
    """(sd_field [...], voxel [...]) of the points x [..., 3]: the header's rule, line by line"""
    x = np.asarray(x, dtype=np.float64)
    n = np.asarray(n)
    u = (x - np.asarray(origin)) / h
    uc = np.clip(u, 0.0, n.astype(np.float64))
    v = np.minimum(np.floor(uc).astype(np.int64), n - 1)
    e = uc - (v + 0.5)
    vox = (v[..., 2] * n[1] + v[..., 1]) * n[0] + v[..., 0]
    q = np.asarray(d2).reshape(-1)[vox]
    with np.errstate(invalid="ignore"):
        sd = h * (np.sqrt(q.astype(np.float64)) - np.linalg.norm(e, axis=-1) - HALF_DIAGONAL)
    return np.where(q == EMPTY, np.inf, sd), vox


def true_distance(origin, h, occ, x):
    """distance of the points x [P, 3] to the union of the occupied cubes (0 inside one), by brute force over the cubes; inf without any"""
    w = np.argwhere(np.asarray(occ) != 0)[:, ::-1]                     # (i, j, k)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    if w.shape[0] == 0:
        return np.full(x.shape[0], np.inf)
    lo = np.asarray(origin) + h * w
    hi = lo + h
    out = np.full(x.shape[0], np.inf)
    for a in range(0, x.shape[0], 256):
        xa = x[a:a + 256, None, :]
        gap = np.maximum(np.maximum(lo[None] - xa, xa - hi[None]), 0.0)
        out[a:a + 256] = np.linalg.norm(gap, axis=2).min(axis=1)
    return out


def rasterise(origin, h, n, obstacles):
    """occupancy of the primitives `obstacles` (capi.OBSTACLE_DTYPE): a voxel is occupied if the signed distance of its centre to some primitive is
    at most h sqrt(3) / 2, which covers every voxel a solid touches"""
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    c = np.asarray(origin) + h * (np.stack([i, j, k], axis=-1) + 0.5)
    occ = np.zeros((n[2], n[1], n[0]), dtype=bool)
    for ob in obstacles:
        occ |= sd_np(ob, c) <= h * HALF_DIAGONAL
    return occ.astype(np.uint8)


def sampled_q(narm, nseg, sx, sT, n_pts):
    """joint positions [B][n_pts + 1][7 narm] at the uniform samples, arm by arm from oracle_py.sample"""
    B, N = sx.shape[0], sx.shape[1]
    q = np.zeros((B, n_pts + 1, 7 * narm))
    for b in range(B):
        for a in range(narm):
            xa = np.concatenate([sx[b][:, 7 * a:7 * a + 7], sx[b][:, 7 * narm + 7 * a:7 * narm + 7 * a + 7]], axis=1)
            q[b, :, 7 * a:7 * a + 7] = o.sample(nseg, xa, np.zeros((N, 7)), sT[b], n_pts)[:, 1:8]
    return q


def field_records(models, tables, origin, h, n, d2, q, sT, n_pts, margin):
    """per problem of q [B][n_pts + 1][7 narm]: the clearances d [S, nsph], the voxels read vox [S, nsph], and the record fields that follow.
    near: some sample minimum within 1e-9 of the margin; fragile: some sphere centre within 1e-9 of an interior voxel face"""
    out = []
    for b in range(q.shape[0]):
        cen, rad, _, _ = sphere_centres(models, tables, q[b])
        S = q.shape[1]
        if cen.shape[1] == 0:
            d, vox, fragile = np.full((S, 0), np.inf), np.zeros((S, 0), dtype=np.int64), False
        else:
            sd, vox = sd_field(origin, h, n, d2, cen)
            d = sd - rad[None, :]
            fragile = bool((face_distance(origin, h, n, cen) <= 1e-9).any())
        smin = d.min(axis=1, initial=np.inf)
        hit = smin < margin
        first = int(np.argmax(hit)) if hit.any() else -1
        out.append(dict(d=d, vox=vox, smin=smin, d_min=smin.min(), n_hit=int(hit.sum()), t_first=(first / n_pts) * sT[b] if first >= 0 else -1.0,
                        status=int(hit.any()), near=bool((np.abs(smin - margin) <= 1e-9).any()), fragile=fragile))
    return out


def merge(a, b):
    """the rule of mpcmp_clearance_merge_batch on two record arrays: (records, source)"""
    out = np.zeros(a.shape[0], dtype=a.dtype)
    src = np.zeros(a.shape[0], dtype=np.int32)
    for i in range(a.shape[0]):
        ra, rb, r = a[i], b[i], out[i]
        r["status"] = ra["status"] | rb["status"]
        if r["status"] & 2:
            r["d_min"] = np.nan; r["t_min"] = -1.0; r["t_first"] = -1.0; r["sphere"] = -1; r["other"] = 0; r["n_hit"] = 0
            continue
        r["n_hit"] = ra["n_hit"] + rb["n_hit"]
        firsts = [t for t in (ra["t_first"], rb["t_first"]) if t >= 0]
        r["t_first"] = min(firsts) if firsts else -1.0
        pick = None
        if ra["sphere"] >= 0:
            pick = 0
        if rb["sphere"] >= 0 and (pick is None or rb["d_min"] < ra["d_min"]):
            pick = 1
        if pick is None:
            r["d_min"] = np.inf; r["t_min"] = -1.0; r["sphere"] = -1; r["other"] = 0
        else:
            w = (ra, rb)[pick]
            r["d_min"] = w["d_min"]; r["t_min"] = w["t_min"]; r["sphere"] = w["sphere"]; r["other"] = w["other"]; src[i] = pick
    return out, src
