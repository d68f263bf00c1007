"""Camera frames as voxel worlds (include/mpcmp_frame.h), the part that needs no GPU: the ABI table and record layouts, the host statements of the
rule (mpcmp_frame_spheres, _points_one, _depth_one, _carve_one) against the NumPy restatement of tests/frame_reference.py, the two clearance
guarantees, every rejection, the sanitized self-test and the kernels' resources.  The builders below (robot, posture, cloud, camera_of, image,
defragile_*) are what tests/test_gpu_frame.py checks the kernels with as well.

Bounds.  Occupancy and counts are integers and compared exactly, which is fair only while no input lies within rounding of a decision: every case
removes the reference's FRAGILE inputs first (tests/frame_reference.py) and asserts ON THE REFERENCE that at most 1 % were removed and that each of
the four classes holds at least 5 % of the frame.  The guarantees are inequalities of the header; they are asserted with 1e-12 of slack for the
rounding of sd_field's own arithmetic (three products and two roots of numbers of order one).

The bound of the points guarantee, pad - (5 sqrt(3) / 2) h, adds two worst cases that exclude each other (the marked cube reaching a whole diagonal
towards the sphere, and sd_field losing (3 sqrt(3) / 2) h on that same cube), so no input attains it.  The worst corner that exists, a point at
R_s + 1e-6 in the far corner of a cube whose diagonal points at a sphere centre that sits in the corner of its own voxel, gives pad - 2 sqrt(3) h:
test_the_points_bound_is_nearly_attained pins that value, half a cube diagonal above the bound, with a pad just below the points threshold."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import field_reference as F
import frame_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ORIGIN = (-1.013, -0.987, -0.131)
GRIDS = {0.04: (50, 50, 36), 0.02: (100, 100, 72)}
Q_ARM = (np.array([0.3, -0.4, 0.2, -1.9, 0.1, 1.7, 0.4]), np.array([-0.5, 0.2, -0.3, -1.5, 0.2, 1.9, -0.6]))
FLOOR_Z, BOX, POLE = -0.05, ((0.6, -0.5, 0.15), (0.1, 0.1, 0.15)), (-0.5, 0.5, 0.04, 0.2, 1.0)
SLACK = 1e-12


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def robot(narm, per_arm=None):
    """(models, tables): the Panda or the two of DUAL_BASES with the skeleton spheres of radius 0.06 at spacing 0.08; per_arm: the first per_arm
    spheres of each table, repeated with shrinking radii up to that number (0, 1 and 64 are the table sizes the kernels must take)"""
    import mpc_motion_planner_amd as M
    models = [M.default_model()] if narm == 1 else list(M.arm_models(M.DUAL_BASES))
    tables = [M.link_spheres(m, 0.06, 0.08) for m in models]
    if per_arm is not None:
        out = []
        for t in tables:
            big = np.concatenate([t] * (per_arm // max(t.shape[0], 1) + 1))[:per_arm].copy()
            big["r"] *= 1.0 - 0.3 * np.arange(per_arm) / max(per_arm, 1)
            out.append(big)
        tables = out
    return models, tables


def posture(narm):
    return np.concatenate(Q_ARM[:narm])


def pad_points(h, margin=0.01):
    return FR.POINTS_BOUND * h + margin + 1e-3


def pad_carve(h, margin=0.01):
    return FR.CARVE_BOUND * h + margin + 1e-3


def cloud(narm, h, pad, n_total=5000, seed=3, tables=None, q=None, models=None):
    """a frame that sees the cell AND the robot: surfaces of the floor, the box and the pole, points beyond the grid, non-finite points and the
    shell of the robot (radius r_s + pad / 2 about every sphere at the capture posture)"""
    mdl, tabs = robot(narm)
    models = mdl if models is None else models
    tabs = tabs if tables is None else tables
    q = posture(narm) if q is None else q
    rng = np.random.default_rng(seed)
    n = GRIDS[h]
    lo, hi = np.asarray(ORIGIN), np.asarray(ORIGIN) + h * np.asarray(n)
    k = [int(0.4 * n_total), int(0.15 * n_total), int(0.1 * n_total)]
    k.append(n_total - sum(k))
    floor = np.column_stack([lo[0] + rng.random(k[0] // 2) * (hi[0] - lo[0]), lo[1] + rng.random(k[0] // 2) * (hi[1] - lo[1]), np.full(k[0] // 2, FLOOR_Z)])
    bc, be = np.asarray(BOX[0]), np.asarray(BOX[1])
    box = bc + (rng.random((k[0] // 4, 3)) * 2 - 1) * be
    ax = rng.integers(3, size=box.shape[0])
    box[np.arange(box.shape[0]), ax] = bc[ax] + be[ax] * rng.choice([-1.0, 1.0], size=box.shape[0])
    m = k[0] - floor.shape[0] - box.shape[0]
    ang = rng.random(m) * 2 * np.pi
    pole = np.column_stack([POLE[0] + POLE[2] * np.cos(ang), POLE[1] + POLE[2] * np.sin(ang), POLE[3] + rng.random(m) * (POLE[4] - POLE[3])])
    beyond = hi + rng.random((k[1], 3)) * 0.5
    beyond[::2] = lo - rng.random(((k[1] + 1) // 2, 3)) * 0.5
    bad = lo + rng.random((k[2], 3)) * (hi - lo)
    bad[np.arange(k[2]), rng.integers(3, size=k[2])] = rng.choice([np.nan, np.inf, -np.inf], size=k[2])
    cen, R = FR.filter_spheres(models, tabs, q, pad / 2)
    if cen.shape[0]:
        s = rng.integers(cen.shape[0], size=k[3])
        d = rng.normal(size=(k[3], 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        shell = cen[s] + R[s, None] * d
    else:
        shell = lo + rng.random((k[3], 3)) * (hi - lo)
    pts = np.concatenate([floor, box, pole, beyond, bad, shell])
    return np.ascontiguousarray(pts[rng.permutation(pts.shape[0])][:n_total])


def camera_of(M, width, height, u16, z_max=3.2):
    R, t = FR.look_at((1.9, -1.5, 1.4), (0.1, 0.1, 0.35))
    return M.camera(R, t, 0.8 * width, 0.8 * width, (width - 1) / 2.0, (height - 1) / 2.0, width, height, depth_scale=0.001 if u16 else 1.0,
                    z_min=0.3, z_max=z_max)


def image(M, narm, width, height, u16, pad, tables=None, q=None, see_robot=True, z_max=3.2):
    """(camera, depth [height][width]) of the scene with the robot as spheres of radius r_s + pad / 2 at the capture posture; nothing hit: 0"""
    models, tabs = robot(narm)
    tabs = tabs if tables is None else tables
    cam = camera_of(M, width, height, u16, z_max)
    cen, R = FR.filter_spheres(models, tabs, posture(narm) if q is None else q, pad / 2)
    z = FR.render(cam, FLOOR_Z, [BOX], [POLE], list(zip(cen, R)) if see_robot else [])
    z = np.where(np.isfinite(z), z, 0.0)
    if u16:
        return cam, np.minimum(np.rint(z * 1000.0), 65535).astype(np.uint16)
    return cam, z.astype(np.float32)


def defragile_points(h, pts, cen, R):
    """(the cloud without the reference's fragile points, how many were dropped)"""
    bad = FR.fragile_points(ORIGIN, h, GRIDS[h], pts, cen, R)
    return np.ascontiguousarray(pts[~bad]), int(bad.sum())


def defragile_image(h, cam, depth, cen, R):
    bad = FR.fragile_pixels(ORIGIN, h, GRIDS[h], cam, depth, cen, R).reshape(depth.shape)
    out = depth.copy(); out[bad] = 0
    return out, int(bad.sum())


def assert_fair(stats, dropped, n_before, classes=True):
    assert dropped <= 0.01 * max(n_before, 1), "reference: %d of %d inputs fragile" % (dropped, n_before)
    assert stats["n_in"] == sum(stats[k] for k in FR.NAMES)
    if classes:
        for k in FR.NAMES:
            assert stats[k] >= 0.05 * stats["n_in"], "reference: class %s holds %d of %d" % (k, stats[k], stats["n_in"])


def as_dict(st):
    return {k: int(st[k]) for k in ("n_in",) + FR.NAMES + ("n_cleared",)}


# ---- layouts and the table --------------------------------------------------------------------------------------------------------------------------
def test_abi_table_matches_the_header_and_the_library(M):
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_frame.h")).read(), flags=re.S)
    decl = []
    for name, args in re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d"}[a.split(" ")[0]]
        decl.append((name, kinds))
    assert len(decl) == 10 and [d[0] for d in decl] == list(capi.ABI_FRAME)
    for name, kinds in decl:
        assert kinds == capi.ABI_FRAME[name], (name, kinds, capi.ABI_FRAME[name])
        f = getattr(M.lib(), name)
        assert f.argtypes == [{"p": C.c_void_p, "i": C.c_int, "d": C.c_double}[k] for k in kinds] and f.restype is C.c_int, name
    main = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert main.index('#include "mpcmp_field.h"') < main.index('#include "mpcmp_frame.h"')
    assert not set(capi.ABI_FRAME) & (set(capi.ABI) | set(capi.ABI_FIELD) | set(capi.ABI_FIELD_CERT))


def test_record_layouts_match_the_header(M, tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", '
                   'sizeof(mpcmp_camera), offsetof(mpcmp_camera, t), offsetof(mpcmp_camera, fx), offsetof(mpcmp_camera, depth_scale), '
                   'offsetof(mpcmp_camera, z_max), offsetof(mpcmp_camera, width), offsetof(mpcmp_camera, height), sizeof(mpcmp_frame_stats), '
                   'offsetof(mpcmp_frame_stats, n_marked), offsetof(mpcmp_frame_stats, n_cleared), MPCMP_DEPTH_U16, MPCMP_DEPTH_F32, MPCMP_FRAME_KEEP); '
                   'return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    c, s = M.CAMERA_DTYPE.fields, M.FRAME_STATS_DTYPE.fields
    assert sz == [160, c["t"][1], c["fx"][1], c["depth_scale"][1], c["z_max"][1], c["width"][1], c["height"][1], 32, s["n_marked"][1], s["n_cleared"][1],
                  M.DEPTH_U16, M.DEPTH_F32, M.FRAME_KEEP], sz
    assert M.CAMERA_DTYPE.itemsize == 160 and M.FRAME_STATS_DTYPE.itemsize == 32 and sz[1:7] == [72, 96, 128, 144, 152, 156]


# ---- the host statements against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm", [1, 2])
def test_filter_spheres_match_the_reference(M, narm):
    models, tables = robot(narm)
    q = posture(narm)
    got = M.frame_spheres(models, tables, q, 0.07)
    cen, R = FR.filter_spheres(models, tables, q, 0.07)
    assert got.shape == (cen.shape[0], 4) and np.abs(got[:, :3] - cen).max() <= 1e-12 and np.array_equal(got[:, 3], R)


@pytest.mark.parametrize("h", sorted(GRIDS))
@pytest.mark.parametrize("narm", [1, 2])
def test_points_match_the_reference(M, narm, h):
    models, tables = robot(narm)
    q, pad, n = posture(narm), pad_points(h), GRIDS[h]
    cen, R = FR.filter_spheres(models, tables, q, pad)
    raw = cloud(narm, h, pad)
    pts, dropped = defragile_points(h, raw, cen, R)
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    assert_fair(ref, dropped, raw.shape[0])
    occ, st = M.frame_points_one(models, tables, M.field_desc(ORIGIN, h, n), pts, q, pad)
    assert as_dict(st) == ref and np.array_equal(occ, ref_occ)
    # no posture: the plain marker
    occ0, st0 = M.frame_points_one(None, None, M.field_desc(ORIGIN, h, n), pts, None, 0.0)
    assert np.array_equal(occ0, F.mark_points(ORIGIN, h, n, pts)) and st0["n_robot"] == 0 and st0["n_marked"] == ref["n_marked"] + ref["n_robot"]
    # KEEP is the OR of two frames
    other = cloud(narm, h, pad, n_total=1500, seed=11)
    other, _ = defragile_points(h, other, cen, R)
    ref_or, ref2 = FR.mark(ORIGIN, h, n, other, cen, R, occ=ref_occ)
    occ2, st2 = M.frame_points_one(models, tables, M.field_desc(ORIGIN, h, n), other, q, pad, keep=True, occ=occ)
    assert as_dict(st2) == ref2 and np.array_equal(occ2, ref_or)
    assert np.array_equal(occ2, ref_occ | FR.mark(ORIGIN, h, n, other, cen, R)[0]) and occ2.sum() > ref_occ.sum()


@pytest.mark.parametrize("u16", [True, False])
@pytest.mark.parametrize("narm,size", [(1, (64, 48)), (2, (70, 37)), (1, (1, 1))])
def test_depth_images_match_the_reference(M, narm, size, u16):
    h = 0.04
    models, tables = robot(narm)
    q, pad, n = posture(narm), pad_points(h), GRIDS[h]
    cen, R = FR.filter_spheres(models, tables, q, pad)
    cam, raw = image(M, narm, size[0], size[1], u16, pad)
    depth, dropped = defragile_image(h, cam, raw, cen, R)
    ref_occ, ref = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R)
    assert_fair(ref, dropped, raw.size, classes=size[0] > 1)
    occ, st = M.frame_depth_one(models, tables, M.field_desc(ORIGIN, h, n), cam, depth, q, pad)
    assert as_dict(st) == ref and np.array_equal(occ, ref_occ)
    print("%d arm(s), %d x %d, %s: %s" % (narm, size[0], size[1], "u16" if u16 else "f32", ref))


@pytest.mark.parametrize("narm,n", [(1, (50, 50, 36)), (2, (33, 31, 29))])
def test_carve_matches_the_reference(M, narm, n):
    h = 0.04
    models, tables = robot(narm)
    q, pad = posture(narm), pad_carve(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    rng = np.random.default_rng(5)
    occ = (rng.random(n[::-1]) < 0.15).astype(np.uint8)
    frag = FR.fragile_voxels(ORIGIN, h, occ, cen, R)
    assert frag.sum() <= 0.01 * occ.size
    occ[frag] = 0
    ref_occ, ref = FR.carve(ORIGIN, h, occ, cen, R)
    got, st = M.frame_carve_one(models, tables, M.field_desc(ORIGIN, h, n), occ, q, pad)
    assert as_dict(st) == ref and np.array_equal(got, ref_occ) and ref["n_cleared"] >= 100 and ref["n_in"] == 0
    assert (np.prod(n) % 4 != 0) == (narm == 2)


# ---- the guarantees -------------------------------------------------------------------------------------------------------------------------------
GUARANTEE_GRID = ((-1.23, -1.21, -0.43), 0.05, (70, 50, 38))     # holds both arms of DUAL_BASES at every posture


@pytest.mark.parametrize("narm", [1, 2])
def test_both_guarantees_over_random_postures(M, narm):
    """200 postures inside the joint ranges: an adversarial cloud (every sphere's shell at R_s + 1e-6, and a dense random cloud) filtered with a pad
    just above 4.34 h + margin, and a full grid carved with a pad just above 3.47 h + margin, leave the capture posture clear by the margin"""
    import oracle_py as o
    origin, h, n = GUARANTEE_GRID
    models, tables = robot(narm)
    desc = M.field_desc(origin, h, n)
    lim = o.default_limits()
    rng = np.random.default_rng(17)
    lo, hi = np.asarray(origin), np.asarray(origin) + h * np.asarray(n)
    margin = 0.01
    pad_p, pad_c = pad_points(h, margin), pad_carve(h, margin)
    worst_p = worst_c = np.inf
    full = np.ones(n[::-1], dtype=np.uint8)
    for it in range(200):
        q = np.tile(lim["qmin"], narm) + rng.random(7 * narm) * np.tile(lim["qmax"] - lim["qmin"], narm)
        cen, R = FR.filter_spheres(models, tables, q, pad_p)
        assert ((cen > lo) & (cen < hi)).all()                            # the guarantee's premise, on the reference
        d = rng.normal(size=(cen.shape[0], 24, 3)); d /= np.linalg.norm(d, axis=2)[:, :, None]
        pts = np.concatenate([(cen[:, None, :] + (R[:, None, None] + 1e-6) * d).reshape(-1, 3), lo + rng.random((3000, 3)) * (hi - lo)])
        occ, st = M.frame_points_one(models, tables, desc, pts, q, pad_p)
        assert st["n_marked"] >= 1000 and st["n_robot"] >= 100
        d_p = M.clearance_field_config(models, tables, desc, M.field_edt(desc, occ), q)[0]
        assert d_p >= pad_p - FR.POINTS_BOUND * h - SLACK and d_p > margin, (it, d_p)
        occ, st = M.frame_carve_one(models, tables, desc, full, q, pad_c)
        assert st["n_cleared"] >= 1000
        d_c = M.clearance_field_config(models, tables, desc, M.field_edt(desc, occ), q)[0]
        assert d_c >= pad_c - FR.CARVE_BOUND * h - SLACK and d_c > margin, (it, d_c)
        worst_p, worst_c = min(worst_p, d_p - (pad_p - FR.POINTS_BOUND * h)), min(worst_c, d_c - (pad_c - FR.CARVE_BOUND * h))
    print("%d arm(s): smallest clearance above the bound: points %.4f (%.2f h), carve %.4f (%.2f h)" % (narm, worst_p, worst_p / h, worst_c, worst_c / h))


def test_the_points_bound_is_nearly_attained(M):
    """one sphere, one point at R_s + 1e-6 along a cube diagonal, the grid laid so that the point sits in the far corner of its cube and the sphere
    centre in the near corner of its own voxel three diagonals away; pad = 4.3 h, just below the points threshold 4.34 h (+ margin 0).  The field
    clearance is pad - 2 sqrt(3) h (the worst a single cube can do), half a diagonal above the bound, and an unfiltered point is a plain hit"""
    m = M.default_model()
    q = Q_ARM[0]
    h0 = 0.05
    pad, r = 4.3 * h0, (3 * np.sqrt(3.0) - 4.3) * h0
    table = M.spheres([5], [[0.0, 0.0, 0.0]], r)
    cen, R = FR.filter_spheres([m], [table], q, pad)
    h = (R[0] + 1e-6) / (3 * np.sqrt(3.0)) * (1 + 1e-7)
    x = cen[0] + (R[0] + 1e-6) * np.ones(3) / np.sqrt(3.0)
    n = (24, 24, 24)
    origin = tuple(x - h * (20 - 1e-7))
    desc = M.field_desc(origin, h, n)
    u_c, u_x = (cen[0] - np.asarray(origin)) / h, (x - np.asarray(origin)) / h
    assert np.all(u_c - 17 > 0) and np.all(u_c - 17 < 1e-6) and np.all(20 - u_x > 0) and np.all(20 - u_x < 1e-6)
    occ, st = M.frame_points_one(m, table, desc, x[None], q, pad)
    assert as_dict(st) == dict(n_in=1, n_invalid=0, n_outside=0, n_robot=0, n_marked=1, n_cleared=0) and occ[19, 19, 19] == 1
    d = M.clearance_field_config(m, table, desc, M.field_edt(desc, occ), q)[0]
    bound = pad - FR.POINTS_BOUND * h
    assert pad < FR.POINTS_BOUND * h + 1e-3 and bound < 0.0
    assert abs(d - (pad - 2 * np.sqrt(3.0) * h)) <= 1e-5 and bound <= d <= bound + np.sqrt(3.0) / 2 * h + 1e-5, (d, bound)
    # one micrometre nearer the point is the robot's own
    occ, st = M.frame_points_one(m, table, desc, (cen[0] + (R[0] - 1e-6) * np.ones(3) / np.sqrt(3.0))[None], q, pad)
    assert st["n_robot"] == 1 and occ.sum() == 0


# ---- rejections -------------------------------------------------------------------------------------------------------------------------------------
def test_every_rejection_writes_nothing(M):
    from mpc_motion_planner_amd.capi import host
    models, tables = robot(1)
    arr = (M.Model * 1)(*[M.Model.from_buffer_copy(m) for m in models])
    tab = np.ascontiguousarray(tables[0]); cnt = np.array([tab.shape[0]], dtype=np.int32)
    h, n = 0.04, (6, 5, 4)
    desc = M.field_desc(ORIGIN, h, n)
    q = np.ascontiguousarray(Q_ARM[0]); pts = np.ascontiguousarray(np.zeros((3, 3)))
    cam = camera_of(M, 4, 3, True); depth = np.full((3, 4), 900, dtype=np.uint16)
    L = M.lib()

    def call(which, **kw):
        occ = np.full(n[::-1], 7, dtype=np.uint8); st = np.zeros((), dtype=M.FRAME_STATS_DTYPE); st["n_in"] = 77
        out = np.full((tab.shape[0], 4), 7.0)
        a = dict(models=arr, narm=1, cnt=host(cnt), tab=host(tab), desc=desc.ctypes.data, n_points=3, points=host(pts), cam=cam.ctypes.data,
                 depth=depth.ctypes.data, depth_type=0, q=host(q), pad=0.1, flags=0, occ=occ.ctypes.data, stats=st.ctypes.data, out=out.ctypes.data)
        a.update(kw)
        if which == "spheres":
            rc = L.mpcmp_frame_spheres(a["models"], a["narm"], a["cnt"], a["tab"], a["q"], a["pad"], a["out"])
        elif which == "points":
            rc = L.mpcmp_frame_points_one(a["models"], a["narm"], a["cnt"], a["tab"], a["desc"], a["n_points"], a["points"], a["q"], a["pad"], a["flags"],
                                          a["occ"], a["stats"])
        elif which == "depth":
            rc = L.mpcmp_frame_depth_one(a["models"], a["narm"], a["cnt"], a["tab"], a["desc"], a["cam"], a["depth"], a["depth_type"], a["q"], a["pad"],
                                         a["flags"], a["occ"], a["stats"])
        else:
            rc = L.mpcmp_frame_carve_one(a["models"], a["narm"], a["cnt"], a["tab"], a["desc"], a["q"], a["pad"], a["occ"], a["stats"])
        return rc, bool(np.all(occ == 7) and st["n_in"] == 77 and np.all(out == 7.0))
    for which in ("spheres", "points", "depth", "carve"):
        assert call(which)[0] == 0, which
    assert call("points", stats=None)[0] == 0 and call("points", q=None, models=None, cnt=None, tab=None)[0] == 0 and call("points", n_points=0, points=None)[0] == 0
    f32, big = np.ones((3, 4), dtype=np.float32), np.zeros((2048, 2048), dtype=np.uint16)
    assert call("points", flags=M.FRAME_KEEP) == (0, False) and call("depth", depth_type=1, depth=f32.ctypes.data)[0] == 0
    bad_cnt = np.array([65], dtype=np.int32)
    bad_tab = tab.copy(); bad_tab["joint"][1] = 7
    bad_q = q.copy(); bad_q[3] = np.nan
    robot_cases = [("no models", dict(models=None)), ("narm 0", dict(narm=0)), ("narm 3", dict(narm=3)), ("no counts", dict(cnt=None)),
                   ("no table", dict(tab=None)), ("65 spheres", dict(cnt=host(bad_cnt))), ("joint 7", dict(tab=host(bad_tab))),
                   ("q NaN", dict(q=host(bad_q))), ("pad < 0", dict(pad=-1e-9)), ("pad NaN", dict(pad=float("nan"))), ("pad inf", dict(pad=float("inf")))]
    bad_n, bad_h, bad_o, bad_v = (M.field_desc(ORIGIN, h, (1025, 1, 1)), M.field_desc(ORIGIN, 0.0, n), M.field_desc((np.nan, 0, 0), h, n),
                                  M.field_desc(ORIGIN, h, (1024, 1024, 17)))
    grid_cases = [("no grid", dict(desc=None)), ("n 1025", dict(desc=bad_n.ctypes.data)), ("h 0", dict(desc=bad_h.ctypes.data)),
                  ("origin NaN", dict(desc=bad_o.ctypes.data)), ("too many voxels", dict(desc=bad_v.ctypes.data)), ("no occ", dict(occ=None))]

    def cam_with(**kw):
        c = cam.copy()
        for k, v in kw.items():
            c[k] = v
        return c
    bad_R = cam.copy(); bad_R["R"][4] = np.inf
    bad_t = cam.copy(); bad_t["t"][1] = np.nan
    cams = [bad_R, bad_t, cam_with(fx=0.0), cam_with(fy=-1.0), cam_with(fx=np.inf), cam_with(cx=np.nan), cam_with(cy=np.inf), cam_with(depth_scale=0.0),
            cam_with(depth_scale=np.nan), cam_with(z_min=-0.1), cam_with(z_min=4.0), cam_with(z_max=np.inf), cam_with(width=0), cam_with(height=0),
            cam_with(width=2049, height=2049)]
    for what, kw in robot_cases + [("no q", dict(q=None)), ("no out", dict(out=None))]:
        assert call("spheres", **kw) == (EINVAL, True), what
    for which in ("points", "depth", "carve"):
        for what, kw in robot_cases + grid_cases:
            assert call(which, **kw) == (EINVAL, True), (which, what)
    for what, kw in (("n_points < 0", dict(n_points=-1)), ("no points", dict(points=None)), ("flag 2", dict(flags=2)), ("flag -1", dict(flags=-1))):
        assert call("points", **kw) == (EINVAL, True), what
    for what, kw in (("no camera", dict(cam=None)), ("no image", dict(depth=None)), ("depth_type 2", dict(depth_type=2)), ("depth_type -1", dict(depth_type=-1)),
                     ("flag 4", dict(flags=4))):
        assert call("depth", **kw) == (EINVAL, True), what
    for i, c in enumerate(cams):
        assert call("depth", cam=c.ctypes.data) == (EINVAL, True), ("camera", i)
    largest = cam_with(width=2048, height=2048)
    assert call("depth", cam=largest.ctypes.data, depth=big.ctypes.data)[0] == 0
    # the calls on a context refuse a missing context without touching a GPU
    assert L.mpcmp_set_field_points_filtered(None, desc.ctypes.data, 0, None, None, 0.0, 0, None) == EINVAL
    assert L.mpcmp_set_field_points_filtered_device(None, desc.ctypes.data, 0, None, None, 0.0, 0, None, None) == EINVAL
    assert L.mpcmp_set_field_depth(None, desc.ctypes.data, cam.ctypes.data, depth.ctypes.data, 0, None, 0.0, 0, None) == EINVAL
    assert L.mpcmp_set_field_depth_device(None, desc.ctypes.data, cam.ctypes.data, depth.ctypes.data, 0, None, 0.0, 0, None, None) == EINVAL
    assert L.mpcmp_field_carve(None, host(q), 0.0, None) == EINVAL and L.mpcmp_field_carve_device(None, host(q), 0.0, None, None) == EINVAL
    assert b"no context" in L.mpcmp_last_error(None)


# ---- the self-test and the kernels' resources -----------------------------------------------------------------------------------------------------
def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/frame_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and UBSan; the
    program checks the class order, the count identity and both guarantees itself"""
    exe = str(tmp_path / "frame_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "frame_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    hst = json.loads(r.stdout.strip().splitlines()[0])["host"]
    assert hst["order_wrong"] == 0 and hst["n_in"] == hst["n_invalid"] + hst["n_outside"] + hst["n_robot"] + hst["n_marked"]
    assert min(hst["n_invalid"], hst["n_outside"], hst["n_robot"], hst["n_marked"]) >= 1
    assert hst["unfiltered_d"] < 0 and hst["points_d"] >= hst["points_bound"] > 0 and hst["carve_d"] >= hst["carve_bound"] > 0 and hst["n_cleared"] > 0
    assert hst["depth_n_in"] == 48 * 36 and hst["depth_n_robot"] > 0 and hst["depth_d"] >= hst["points_bound"]


def test_frame_kernels_use_no_scratch():
    """the compiler's resource remarks of frame.hip, by the mechanism of tests/test_kernel_resources.py (hipcc cross-compiles: no GPU needed)"""
    import tempfile
    import test_kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        proc, _ = kr._compile("frame.hip", [], tmp, "frm")
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        res = {k: v for k, v in kr._resources(err).items() if k.startswith("_ZN5mpcmp")}
        assert len(res) == 5 and sum("k_frame_mark" in k for k in res) == 3 and sum("k_frame_spheres" in k for k in res) == 1 and \
            sum("k_frame_carve" in k for k in res) == 1, list(res)
        for k, v in res.items():
            print("%s: %d VGPRs, %d B of scratch per lane" % (k, v["vgpr"], v["scratch"]))
            assert v["scratch"] == 0 and v["vgpr"] <= 128, (k, v)
