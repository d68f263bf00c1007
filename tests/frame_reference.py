"""NumPy reference of the camera frames (include/mpcmp_frame.h).  It shares nothing with the library: the classes, the pixel rule, the carve rule and
the counts are written out from the header on the forward kinematics of tests/test_clearance_host.py (sphere_centres) and the marker and transform
of tests/field_reference.py (mark_points, edt).  A tiny ray caster renders the depth image a camera would see of a scene of a floor, a box, a pole
and the robot as spheres, the nearest hit per pixel.

FRAGILE inputs, where rounding may legitimately put the library on the other side of a decision: a point within 1e-9 of a voxel face, a point within
1e-9 of a filter sphere's surface, a pixel whose z lies within 1e-9 of z_min or z_max, and for carving a voxel centre within 1e-9 of a filter sphere's
surface.  The tests drop them from their inputs."""
import numpy as np

import field_reference as F
from test_clearance_host import sphere_centres

INVALID, OUTSIDE, ROBOT, MARKED = 0, 1, 2, 3
NAMES = ("n_invalid", "n_outside", "n_robot", "n_marked")
EPS = 1e-9
POINTS_BOUND = 2.5 * np.sqrt(3.0)        # clearance at q >= pad - POINTS_BOUND h for a field built from filtered points
CARVE_BOUND = 2.0 * np.sqrt(3.0)         # ... >= pad - CARVE_BOUND h after a carve


def filter_spheres(models, tables, q, pad):
    """(centres [ns][3], filter radii R_s = r_s + pad [ns]) at the posture q [7 narm]; q None: no sphere"""
    if q is None:
        return np.zeros((0, 3)), np.zeros(0)
    cen, rad, _, _ = sphere_centres(models, tables, np.asarray(q, dtype=np.float64))
    return cen.reshape(-1, 3), rad + pad


def in_robot(x, cen, R):
    """|x - c_s|^2 <= R_s^2 for some s, for the points x [P][3]"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(x.shape[0], dtype=bool)
    for c, r in zip(cen, R):
        d = x - c
        out |= (d * d).sum(axis=1) <= r * r
    return out


def classify(origin, h, n, points, cen, R, invalid=None):
    """the class of every point [P]: the four tests in the header's order; invalid [P]: points that are INVALID for a reason of their own (pixels)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cls = np.full(p.shape[0], MARKED)
    with np.errstate(invalid="ignore"):
        u = (p - np.asarray(origin)) / h
        inside = (u >= 0).all(axis=1) & (u < np.asarray(n)).all(axis=1)
        rob = in_robot(p, cen, R)
    bad = ~np.isfinite(p).all(axis=1)
    if invalid is not None:
        bad |= invalid
    cls[rob] = ROBOT
    cls[~inside] = OUTSIDE
    cls[bad] = INVALID
    return cls


def counts(cls, n_cleared=0):
    d = {"n_in": int(cls.shape[0]), "n_cleared": int(n_cleared)}
    for k, nm in enumerate(NAMES):
        d[nm] = int((cls == k).sum())
    return d


def mark(origin, h, n, points, cen, R, occ=None, invalid=None):
    """(occupancy [n2][n1][n0], counts) of a frame of points; occ: the occupancy to keep (MPCMP_FRAME_KEEP)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cls = classify(origin, h, n, p, cen, R, invalid)
    new = F.mark_points(origin, h, n, p[cls == MARKED])
    if occ is not None:
        new = ((np.asarray(occ) != 0) | (new != 0)).astype(np.uint8)
    return new, counts(cls)


def pixel_points(cam, depth):
    """(world points [H W][3], invalid [H W], z [H W]) of a depth image by the header's pixel rule; cam: a record with the fields of mpcmp_camera"""
    W, H = int(cam["width"]), int(cam["height"])
    d = np.asarray(depth).reshape(H * W)
    if d.dtype == np.uint16:
        raw_bad = d == 0
    else:
        d = d.astype(np.float32)
        with np.errstate(invalid="ignore"):
            raw_bad = ~np.isfinite(d) | (d <= 0)
    with np.errstate(invalid="ignore", over="ignore"):
        z = d.astype(np.float64) * float(cam["depth_scale"])
        bad = raw_bad | (z < float(cam["z_min"])) | (z > float(cam["z_max"]))
        v, u = np.divmod(np.arange(H * W), W)
        p = np.stack([z * (u - float(cam["cx"])) / float(cam["fx"]), z * (v - float(cam["cy"])) / float(cam["fy"]), z], axis=1)
        x = p @ np.asarray(cam["R"], dtype=np.float64).reshape(3, 3).T + np.asarray(cam["t"], dtype=np.float64)
    x[bad] = np.nan
    return x, bad, z


def mark_depth(origin, h, n, cam, depth, cen, R, occ=None):
    x, bad, _ = pixel_points(cam, depth)
    return mark(origin, h, n, x, cen, R, occ, invalid=bad)


def voxel_centres(origin, h, n):
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return np.asarray(origin) + h * (np.stack([i, j, k], axis=-1) + 0.5)


def carve(origin, h, occ, cen, R):
    """(occupancy with the occupied voxels whose centre lies in a filter sphere cleared, counts)"""
    occ = (np.asarray(occ) != 0)
    n = occ.shape[::-1]
    hit = in_robot(voxel_centres(origin, h, n).reshape(-1, 3), cen, R).reshape(occ.shape) & occ
    return (occ & ~hit).astype(np.uint8), counts(np.zeros(0, dtype=int), hit.sum())


# ---- fragile inputs -----------------------------------------------------------------------------------------------------------------------------
def near_surface(x, cen, R):
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(x.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for c, r in zip(cen, R):
            out |= np.abs(np.linalg.norm(x - c, axis=1) - r) <= EPS
    return out


def fragile_points(origin, h, n, points, cen, R):
    """[P] bool: within 1e-9 of a voxel face (the grid's outer faces included) or of a filter sphere's surface"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        u = (p - np.asarray(origin)) / h
        face = (np.abs(u - np.rint(u)) * h <= EPS).any(axis=1)
    return (face | near_surface(p, cen, R)) & np.isfinite(p).all(axis=1)


def fragile_pixels(origin, h, n, cam, depth, cen, R):
    x, bad, z = pixel_points(cam, depth)
    with np.errstate(invalid="ignore"):
        edge = (np.abs(z - float(cam["z_min"])) <= EPS) | (np.abs(z - float(cam["z_max"])) <= EPS)
    return (fragile_points(origin, h, n, x, cen, R) & ~bad) | (edge & np.isfinite(z))


def fragile_voxels(origin, h, occ, cen, R):
    occ = np.asarray(occ)
    return near_surface(voxel_centres(origin, h, occ.shape[::-1]).reshape(-1, 3), cen, R).reshape(occ.shape)


# ---- a tiny ray caster --------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """(R [3][3] camera to world, t [3]) of a camera at `eye` whose z axis points at `target`, x to the right, y down"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye; z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, dtype=np.float64)); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z], axis=1), eye


def render(cam, floor_z=None, boxes=(), poles=(), spheres=()):
    """depth z [H][W] (float64, +inf where nothing is hit) of the scene seen by cam: the nearest hit per pixel.  floor_z: the plane z = floor_z;
    boxes: (centre [3], half extents [3]); poles: (x, y, radius, z_lo, z_hi) vertical cylinders without caps; spheres: (centre [3], radius).
    A ray is t + z R ((u - cx) / fx, (v - cy) / fy, 1): its parameter is the depth itself"""
    W, H = int(cam["width"]), int(cam["height"])
    v, u = np.divmod(np.arange(H * W), W)
    dc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]), (v - float(cam["cy"])) / float(cam["fy"]), np.ones(H * W)], axis=1)
    d = dc @ np.asarray(cam["R"], dtype=np.float64).reshape(3, 3).T
    o = np.asarray(cam["t"], dtype=np.float64)
    best = np.full(H * W, np.inf)

    def take(z, ok):
        nonlocal best
        z = np.where(ok & (z > 1e-6), z, np.inf)
        best = np.minimum(best, z)
    with np.errstate(divide="ignore", invalid="ignore"):
        if floor_z is not None:
            take((floor_z - o[2]) / d[:, 2], np.ones(H * W, dtype=bool))
        for c, e in boxes:
            lo, hi = (np.asarray(c) - np.asarray(e) - o) / d, (np.asarray(c) + np.asarray(e) - o) / d
            t0, t1 = np.minimum(lo, hi).max(axis=1), np.maximum(lo, hi).min(axis=1)
            take(t0, t0 <= t1)
        for px, py, r, z_lo, z_hi in poles:
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            b = d[:, 0] * (o[0] - px) + d[:, 1] * (o[1] - py)
            disc = b * b - a * ((o[0] - px) ** 2 + (o[1] - py) ** 2 - r * r)
            z = (-b - np.sqrt(disc)) / a
            zw = o[2] + z * d[:, 2]
            take(z, (disc >= 0) & (zw >= z_lo) & (zw <= z_hi))
        for c, r in spheres:
            oc = o - np.asarray(c)
            a = (d * d).sum(axis=1)
            b = d @ oc
            disc = b * b - a * (oc @ oc - r * r)
            take((-b - np.sqrt(disc)) / a, disc >= 0)
    return best.reshape(H, W)
