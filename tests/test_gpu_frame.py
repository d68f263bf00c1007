"""Camera frames as voxel worlds on the GPU (include/mpcmp_frame.h): k_frame_spheres, k_frame_mark over its three sources and k_frame_carve against
tests/frame_reference.py (the header's rule in NumPy, SciPy's exact transform), with the builders of tests/test_frame_host.py.

Bounds.  The field (mpcmp_get_field) and the counts are integers: bit-exact.  That is fair only while no input lies within rounding of a decision, so
before each call the test removes the reference's FRAGILE inputs (a point is dropped, a pixel zeroed, a voxel emptied) and asserts ON THE REFERENCE
that at most 1 % were removed; the parity cases also assert that each of the four classes holds at least 5 % of the frame.  Clearances of the
closing cases: 1e-10 against the reference, the bound of tests/test_gpu_field.py (check_records is that file's)."""
import json
import os
import subprocess

import numpy as np
import pytest

import field_reference as F
import frame_reference as FR
import test_frame_host as H
from test_gpu_clearance import MARGINS
from test_gpu_field import check_records

pytestmark = pytest.mark.gpu

ORIGIN, GRIDS, ROOT = H.ORIGIN, H.GRIDS, H.ROOT
EINVAL = -1


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def solver(M, narm, tables, B=4, models=None):
    if models is None:
        models = M.arm_models(M.DUAL_BASES) if narm == 2 else None
        s = M.Solver(M.default_config(6 if narm == 2 else 4, 1, margins=MARGINS), B, models=models)      # (two arms: num_seg 6 or 8)
    else:
        s = M.Solver(M.default_config(4, 1, margins=MARGINS), B, model=models[0])
    for a in range(narm):
        s.set_robot_spheres(tables[a], arm=a)
    return s


def field_of(s):
    return s.field()[1]


def check_field(s, ref_occ, what=""):
    d2 = field_of(s)
    assert np.array_equal(d2 == 0, ref_occ != 0), (what, int(((d2 == 0) != (ref_occ != 0)).sum()))
    assert np.array_equal(d2, F.edt(ref_occ)), what


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", sorted(GRIDS))
@pytest.mark.parametrize("narm", [1, 2])
def test_cloud_parity_with_the_reference(M, narm, h):
    models, tables = H.robot(narm)
    q, pad, n = H.posture(narm), H.pad_points(h), GRIDS[h]
    cen, R = FR.filter_spheres(models, tables, q, pad)
    raw = H.cloud(narm, h, pad)
    pts, dropped = H.defragile_points(h, raw, cen, R)
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    H.assert_fair(ref, dropped, raw.shape[0])
    s = solver(M, narm, tables)
    got = s.set_field_points_filtered(M.field_desc(ORIGIN, h, n), pts, q, pad)
    print("arms %d, h %.2f: %s, %d dropped" % (narm, h, got, dropped))
    assert got == ref
    check_field(s, ref_occ)
    s.close()


@pytest.mark.parametrize("u16", [True, False])
@pytest.mark.parametrize("narm,h,size", [(1, 0.04, (64, 48)), (2, 0.02, (70, 37)), (1, 0.04, (1, 1))])
def test_depth_parity_with_the_reference(M, narm, h, size, u16):
    models, tables = H.robot(narm)
    q, pad, n = H.posture(narm), H.pad_points(h), GRIDS[h]
    cen, R = FR.filter_spheres(models, tables, q, pad)
    cam, raw = H.image(M, narm, size[0], size[1], u16, pad)
    depth, dropped = H.defragile_image(h, cam, raw, cen, R)
    ref_occ, ref = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R)
    H.assert_fair(ref, dropped, raw.size, classes=size[0] > 1)
    s = solver(M, narm, tables)
    got = s.set_field_depth(M.field_desc(ORIGIN, h, n), cam, depth, q, pad)
    print("arms %d, h %.2f, %d x %d %s: %s, %d zeroed" % (narm, h, size[0], size[1], "u16" if u16 else "f32", got, dropped))
    assert got == ref
    check_field(s, ref_occ)
    s.close()


@pytest.mark.parametrize("narm,h,n", [(1, 0.04, (50, 50, 36)), (2, 0.04, (33, 31, 29)), (1, 0.02, (100, 100, 72))])
def test_carve_parity_with_the_reference(M, narm, h, n):
    """(33 x 31 x 29 = 29667 voxels: no multiple of four, the last lane takes three bytes)"""
    models, tables = H.robot(narm)
    q, pad = H.posture(narm), H.pad_carve(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    occ = (np.random.default_rng(5).random(n[::-1]) < 0.15).astype(np.uint8)
    occ.reshape(-1)[-3:] = 1
    frag = FR.fragile_voxels(ORIGIN, h, occ, cen, R)
    assert frag.sum() <= 0.01 * occ.size
    occ[frag] = 0
    ref_occ, ref = FR.carve(ORIGIN, h, occ, cen, R)
    assert ref["n_cleared"] >= 100
    s = solver(M, narm, tables)
    s.set_field(M.field_desc(ORIGIN, h, n), occ)
    got = s.field_carve(q, pad)
    assert got == ref
    check_field(s, ref_occ)
    # carving twice clears nothing more
    assert s.field_carve(q, pad)["n_cleared"] == 0
    check_field(s, ref_occ)
    s.close()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------------------------
def test_every_cloud_size(M):
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(1)
    q, pad = H.posture(1), H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    pts, _ = H.defragile_points(h, H.cloud(1, h, pad), cen, R)
    s = solver(M, 1, tables)
    desc = M.field_desc(ORIGIN, h, n)
    for k in (0, 1, 63, 64, 65, 255, 256, 257, 5000):
        sub = np.ascontiguousarray(pts[:k] if k < 5000 else np.concatenate([pts, pts])[:5000])
        ref_occ, ref = FR.mark(ORIGIN, h, n, sub, cen, R)
        assert s.set_field_points_filtered(desc, sub, q, pad) == ref, k
        check_field(s, ref_occ, k)
    s.close()


@pytest.mark.parametrize("narm,per_arm", [(1, 0), (1, 1), (1, 64), (2, 0), (2, 1), (2, 64)])
def test_sphere_table_sizes(M, narm, per_arm):
    """0, 1 and 64 spheres per arm (128 on two arms): cloud, image and carve"""
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(narm, per_arm)
    q, pad = H.posture(narm), H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    assert cen.shape[0] == narm * per_arm
    s = solver(M, narm, tables)
    desc = M.field_desc(ORIGIN, h, n)
    pts, dropped = H.defragile_points(h, H.cloud(narm, h, pad, n_total=2000, tables=tables), cen, R)
    assert dropped <= 20
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    assert s.set_field_points_filtered(desc, pts, q, pad) == ref and (ref["n_robot"] > 0) == (per_arm > 0)
    check_field(s, ref_occ, "cloud")
    cam, raw = H.image(M, narm, 64, 48, True, pad, tables=tables)
    depth, dropped = H.defragile_image(h, cam, raw, cen, R)
    assert dropped <= 30
    ref_occ, ref = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R)
    assert s.set_field_depth(desc, cam, depth, q, pad) == ref
    check_field(s, ref_occ, "image")
    occ = (np.random.default_rng(8).random(n[::-1]) < 0.1).astype(np.uint8)
    occ[FR.fragile_voxels(ORIGIN, h, occ, cen, R)] = 0
    ref_occ, ref = FR.carve(ORIGIN, h, occ, cen, R)
    s.set_field(desc, occ)
    assert s.field_carve(q, pad) == ref and (ref["n_cleared"] > 0) == (per_arm > 0)
    check_field(s, ref_occ, "carve")
    s.close()


def test_keep_after_a_cloud_and_after_set_field(M):
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(1)
    q, pad = H.posture(1), H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    desc = M.field_desc(ORIGIN, h, n)
    a, _ = H.defragile_points(h, H.cloud(1, h, pad, n_total=3000, seed=21), cen, R)
    b, _ = H.defragile_points(h, H.cloud(1, h, pad, n_total=3000, seed=22), cen, R)
    s = solver(M, 1, tables)
    occ_a, _ = FR.mark(ORIGIN, h, n, a, cen, R)
    occ_ab, ref_b = FR.mark(ORIGIN, h, n, b, cen, R, occ=occ_a)
    s.set_field_points_filtered(desc, a, q, pad)
    assert s.set_field_points_filtered(desc, b, q, pad, keep=True) == ref_b
    check_field(s, occ_ab, "cloud + cloud")
    assert occ_ab.sum() > occ_a.sum()
    # a camera on top of a static map, then a depth camera on top of both
    static = (np.random.default_rng(4).random(n[::-1]) < 0.01).astype(np.uint8)
    s.set_field(desc, static)
    occ_sb, _ = FR.mark(ORIGIN, h, n, b, cen, R, occ=static)
    assert s.set_field_points_filtered(desc, b, q, pad, keep=True) == ref_b
    check_field(s, occ_sb, "map + cloud")
    cam, raw = H.image(M, 1, 64, 48, False, pad)
    depth, _ = H.defragile_image(h, cam, raw, cen, R)
    occ_sbd, ref_d = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R, occ=occ_sb)
    assert s.set_field_depth(desc, cam, depth, q, pad, keep=True) == ref_d
    check_field(s, occ_sbd, "map + cloud + image")
    # KEEP on another grid, or without a field: refused, nothing changes
    L = M.lib()
    other = M.field_desc(ORIGIN, h, (50, 50, 35))
    st = np.zeros((), dtype=M.FRAME_STATS_DTYPE); st["n_in"] = 77
    assert L.mpcmp_set_field_points_filtered(s._ctx, other.ctypes.data, b.shape[0], b.ctypes.data, q.ctypes.data, pad, M.FRAME_KEEP, st.ctypes.data) == EINVAL
    assert st["n_in"] == 77
    check_field(s, occ_sbd, "after a refusal")
    s.set_field(None)
    assert L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, b.shape[0], b.ctypes.data, q.ctypes.data, pad, M.FRAME_KEEP, None) == EINVAL
    assert L.mpcmp_field_carve(s._ctx, q.ctypes.data, pad, st.ctypes.data) == EINVAL and st["n_in"] == 77
    with pytest.raises(M.MpcmpError):
        s.field()
    s.close()


def test_rejections_on_a_context_change_nothing(M):
    h, n = 0.04, (12, 10, 8)
    models, tables = H.robot(1)
    s = solver(M, 1, tables)
    desc = M.field_desc(ORIGIN, h, n)
    occ = (np.random.default_rng(2).random(n[::-1]) < 0.2).astype(np.uint8)
    s.set_field(desc, occ)
    L, q = M.lib(), np.ascontiguousarray(H.posture(1))
    pts = np.zeros((3, 3)); cam = H.camera_of(M, 4, 3, True); depth = np.full((3, 4), 900, dtype=np.uint16)
    bad_q = q.copy(); bad_q[2] = np.inf
    bad_cam = cam.copy(); bad_cam["fx"] = 0.0
    bad_desc = M.field_desc(ORIGIN, 0.0, n)
    st = np.zeros((), dtype=M.FRAME_STATS_DTYPE); st["n_in"] = 77
    sp = st.ctypes.data
    for rc in (L.mpcmp_set_field_points_filtered(s._ctx, None, 3, pts.ctypes.data, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, bad_desc.ctypes.data, 3, pts.ctypes.data, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, 3, None, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, -1, pts.ctypes.data, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, 3, pts.ctypes.data, bad_q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, 3, pts.ctypes.data, q.ctypes.data, -0.1, 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, 3, pts.ctypes.data, q.ctypes.data, float("nan"), 0, sp),
               L.mpcmp_set_field_points_filtered(s._ctx, desc.ctypes.data, 3, pts.ctypes.data, q.ctypes.data, 0.1, 2, sp),
               L.mpcmp_set_field_depth(s._ctx, desc.ctypes.data, None, depth.ctypes.data, 0, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_depth(s._ctx, desc.ctypes.data, bad_cam.ctypes.data, depth.ctypes.data, 0, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_depth(s._ctx, desc.ctypes.data, cam.ctypes.data, None, 0, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_depth(s._ctx, desc.ctypes.data, cam.ctypes.data, depth.ctypes.data, 2, q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_set_field_depth(s._ctx, desc.ctypes.data, cam.ctypes.data, depth.ctypes.data, 0, bad_q.ctypes.data, 0.1, 0, sp),
               L.mpcmp_field_carve(s._ctx, bad_q.ctypes.data, 0.1, sp), L.mpcmp_field_carve(s._ctx, q.ctypes.data, -1.0, sp),
               L.mpcmp_field_carve_device(s._ctx, q.ctypes.data, float("inf"), None, None)):
        assert rc == EINVAL
    assert st["n_in"] == 77
    check_field(s, occ, "after the refusals")
    # no posture: nothing is carved, and stats may be NULL
    assert s.field_carve(None, 0.1)["n_cleared"] == 0
    assert L.mpcmp_field_carve(s._ctx, q.ctypes.data, 0.1, None) == 0
    s.close()


def test_a_robot_that_is_not_the_panda(M, tmp_path):
    from robots import general_models
    h, n = 0.04, GRIDS[0.04]
    models = [general_models(M, tmp_path, 31, 1)[0][0]]
    tables = [M.link_spheres(models[0], 0.05, 0.07)]
    q = np.array([0.4, -0.7, 0.5, -1.2, 0.3, 1.1, -0.2])
    pad = H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    assert np.abs(M.frame_spheres(models, tables, q, pad)[:, :3] - cen).max() <= 1e-12
    raw = H.cloud(1, h, pad, tables=tables, q=q, models=models)
    pts, dropped = H.defragile_points(h, raw, cen, R)
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    assert dropped <= 50 and ref["n_robot"] >= 250 and ref["n_marked"] >= 250
    s = solver(M, 1, tables, models=models)
    assert s.set_field_points_filtered(M.field_desc(ORIGIN, h, n), pts, q, pad) == ref
    check_field(s, ref_occ)
    s.close()


def test_no_posture_is_set_field_points(M):
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(1)
    pts = H.cloud(1, h, 0.1)
    s = solver(M, 1, tables)
    desc = M.field_desc(ORIGIN, h, n)
    s.set_field_points(desc, pts)
    plain = field_of(s)
    got = s.set_field_points_filtered(desc, pts, None, 0.0)
    assert field_of(s).tobytes() == plain.tobytes() and got["n_robot"] == 0 and got["n_in"] == pts.shape[0] == sum(got[k] for k in FR.NAMES)
    s.close()


def test_device_variants_on_a_callers_stream(M):
    import torch
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(2)
    q, pad = H.posture(2), H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    pts, _ = H.defragile_points(h, H.cloud(2, h, pad), cen, R)
    cam, raw = H.image(M, 2, 70, 37, True, pad)
    depth, _ = H.defragile_image(h, cam, raw, cen, R)
    camf, rawf = H.image(M, 2, 70, 37, False, pad)
    depthf, _ = H.defragile_image(h, camf, rawf, cen, R)
    desc = M.field_desc(ORIGIN, h, n)
    s = solver(M, 2, tables)
    st = torch.cuda.Stream()

    def stats_of(t):
        return H.as_dict(np.frombuffer(t.cpu().numpy().tobytes(), dtype=M.FRAME_STATS_DTYPE)[0])
    with torch.cuda.stream(st):
        dp = torch.from_numpy(pts).cuda()
        dd, ddf = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(depthf).cuda()
        ds = [torch.full((32,), 9, dtype=torch.uint8, device="cuda") for _ in range(4)]
        s.set_field_points_filtered_device(desc, pts.shape[0], dp.data_ptr(), q, pad, stats=ds[0].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    assert stats_of(ds[0]) == ref
    check_field(s, ref_occ, "cloud")
    with torch.cuda.stream(st):
        s.set_field_depth_device(desc, cam, dd.data_ptr(), M.DEPTH_U16, q, pad, keep=True, stats=ds[1].data_ptr(), stream=st.cuda_stream)
        s.set_field_depth_device(desc, camf, ddf.data_ptr(), M.DEPTH_F32, q, pad, keep=True, stream=st.cuda_stream)      # (no stats)
    st.synchronize()
    ref_occ, ref = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R, occ=ref_occ)
    assert stats_of(ds[1]) == ref
    ref_occ, _ = FR.mark_depth(ORIGIN, h, n, camf, depthf, cen, R, occ=ref_occ)
    check_field(s, ref_occ, "cloud + two images")
    cen_c, R_c = FR.filter_spheres(models, tables, q, H.pad_carve(h))
    occ = (np.random.default_rng(9).random(n[::-1]) < 0.1).astype(np.uint8)
    occ[FR.fragile_voxels(ORIGIN, h, occ, cen_c, R_c)] = 0
    with torch.cuda.stream(st):
        docc = torch.from_numpy(occ).cuda()
        s.set_field_device(desc, docc.data_ptr(), stream=st.cuda_stream)
        s.field_carve_device(q, H.pad_carve(h), stats=ds[2].data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    ref_occ, ref = FR.carve(ORIGIN, h, occ, cen_c, R_c)
    assert stats_of(ds[2]) == ref and ref["n_cleared"] >= 100
    check_field(s, ref_occ, "carve")
    assert torch.equal(ds[3].cpu(), torch.full((32,), 9, dtype=torch.uint8))
    s.close()


# ---- 3. the point of it all ---------------------------------------------------------------------------------------------------------------------
N_PTS, MARGIN = 100, 0.01
Q_GOAL = np.array([2.6, 0.75, 0.0, -1.0, 0.0, 1.8, 0.4])          # a sweep from the capture posture across the pole at (-0.5, 0.5)


def plan_from_the_capture_posture():
    import oracle_py as o
    lim = o.default_limits()
    x0, xf = np.concatenate([H.Q_ARM[0], np.zeros(7)]), np.concatenate([Q_GOAL, np.zeros(7)])
    sx, _, sT = o.warm_start_jerk(4, MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"], x0, xf)
    return sx[None], np.array([sT])


def frame_that_sees_the_robot(M, h, with_pole=True):
    """(camera, depth, the filter spheres for pad_points(h)) of a 160 x 120 frame of the cell with the robot in it"""
    models, tables = H.robot(1)
    pad = H.pad_points(h, MARGIN)
    cam = H.camera_of(M, 160, 120, False, z_max=4.5)
    cen, R = FR.filter_spheres(models, tables, H.posture(1), pad / 2)
    z = FR.render(cam, H.FLOOR_Z, [H.BOX], [H.POLE] if with_pole else [], list(zip(cen, R)))
    depth = np.where(np.isfinite(z), z, 0.0).astype(np.float32)
    cen, R = FR.filter_spheres(models, tables, H.posture(1), pad)
    bad = FR.fragile_pixels(ORIGIN, h, GRIDS[h], cam, depth, cen, R).reshape(depth.shape)
    assert bad.sum() <= 0.01 * depth.size
    depth[bad] = 0
    return cam, depth, cen, R, pad


def reference_records(h, occ, sx, sT):
    models, tables = H.robot(1)
    return F.field_records(models, tables, ORIGIN, h, GRIDS[h], F.edt(occ), F.sampled_q(1, 4, sx, sT, N_PTS), sT, N_PTS, MARGIN)


def test_a_frame_that_sees_the_robot(M):
    """unfiltered, the plan that starts at the capture posture hits at sample 0 with d_min < 0; filtered, or carved out of the unfiltered grid, the
    first sample is clear by the derived bound and the pole still gives the hit the reference predicts later; the certified check agrees, and
    without the pole the plan is certified clear"""
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(1)
    sx, sT = plan_from_the_capture_posture()
    cam, depth, cen, R, pad = frame_that_sees_the_robot(M, h)
    desc = M.field_desc(ORIGIN, h, n)
    s = solver(M, 1, tables)
    # unfiltered
    occ_raw, _ = FR.mark_depth(ORIGIN, h, n, cam, depth, np.zeros((0, 3)), np.zeros(0))
    ref_raw = reference_records(h, occ_raw, sx, sT)
    assert ref_raw[0]["smin"][0] < 0.0 and not ref_raw[0]["fragile"]
    st = s.set_field_depth(desc, cam, depth)
    assert st["n_robot"] == 0
    check_field(s, occ_raw, "unfiltered")
    raw = s.clearance_field(sx, sT, N_PTS, MARGIN)
    check_records(raw, ref_raw, sT, N_PTS, "unfiltered")
    assert raw[0]["status"] & M.CLR_HIT and raw[0]["t_first"] == 0.0 and raw[0]["d_min"] < 0.0
    # filtered
    occ_f, ref_st = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R)
    ref_f = reference_records(h, occ_f, sx, sT)
    bound = pad - FR.POINTS_BOUND * h
    assert bound > MARGIN and ref_f[0]["smin"][0] >= bound and ref_f[0]["n_hit"] >= 1 and ref_f[0]["t_first"] > 0.0 and not ref_f[0]["fragile"]
    assert s.set_field_depth(desc, cam, depth, H.posture(1), pad) == ref_st and ref_st["n_robot"] >= 500
    check_field(s, occ_f, "filtered")
    got = s.clearance_field(sx, sT, N_PTS, MARGIN)
    check_records(got, ref_f, sT, N_PTS, "filtered")
    first = s.clearance_field(sx, sT, 1, MARGIN)                      # (two samples: the start and the goal)
    start = M.clearance_field_config(models, tables, desc, F.edt(occ_f), H.posture(1))[0]
    assert start >= bound and got[0]["t_first"] > 0.0 and got[0]["status"] & M.CLR_HIT and first[0]["d_min"] <= start + 1e-10
    voxel = int(got[0]["other"])
    pole_xy = np.asarray(ORIGIN)[:2] + h * (np.array([voxel % n[0], voxel // n[0] % n[1]]) + 0.5)
    assert np.linalg.norm(pole_xy - np.asarray(H.POLE[:2])) <= H.POLE[2] + 2 * h          # the voxel of d_min is the pole's
    clr, cert = s.clearance_certified_field(sx, sT, MARGIN, 4, 10)
    assert clr[0]["status"] & M.CLR_HIT and clr[0]["t_first"] > 0.0 and clr[0]["d_min"] <= got[0]["d_min"] + 1e-10
    # the unfiltered grid from elsewhere, carved
    pad_c = H.pad_carve(h, MARGIN)
    cen_c, R_c = FR.filter_spheres(models, tables, H.posture(1), pad_c)
    assert not FR.fragile_voxels(ORIGIN, h, occ_raw, cen_c, R_c)[occ_raw != 0].any()
    occ_c, ref_c = FR.carve(ORIGIN, h, occ_raw, cen_c, R_c)
    ref_cr = reference_records(h, occ_c, sx, sT)
    assert ref_cr[0]["smin"][0] >= pad_c - FR.CARVE_BOUND * h > MARGIN and ref_cr[0]["n_hit"] >= 1 and not ref_cr[0]["fragile"]
    s.set_field(desc, occ_raw)
    assert s.field_carve(H.posture(1), pad_c) == ref_c and ref_c["n_cleared"] >= 100
    check_field(s, occ_c, "carved")
    carved = s.clearance_field(sx, sT, N_PTS, MARGIN)
    check_records(carved, ref_cr, sT, N_PTS, "carved")
    assert carved[0]["t_first"] > 0.0 and carved[0]["status"] & M.CLR_HIT
    # without the pole: certified clear
    cam, depth, cen, R, pad = frame_that_sees_the_robot(M, h, with_pole=False)
    occ_n, _ = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R)
    assert reference_records(h, occ_n, sx, sT)[0]["n_hit"] == 0
    s.set_field_depth(desc, cam, depth, H.posture(1), pad)
    check_field(s, occ_n, "no pole")
    clr, cert = s.clearance_certified_field(sx, sT, MARGIN, 4, 10)
    assert clr[0]["status"] == 0 and cert[0]["d_lower"] >= MARGIN
    s.set_field_depth(desc, cam, depth)
    assert s.clearance_certified_field(sx, sT, MARGIN, 4, 10)[0][0]["status"] & M.CLR_HIT
    s.close()


# ---- 4. façade and shim -------------------------------------------------------------------------------------------------------------------------
def test_planner_facade_and_the_cpp_shim(M, tmp_path):
    h, n = 0.04, GRIDS[0.04]
    models, tables = H.robot(1)
    q = H.posture(1)
    pad = H.pad_points(h)
    cen, R = FR.filter_spheres(models, tables, q, pad)
    p = M.BatchMotionPlanner(max_batch=2, num_seg=4, sqp_iters=2)
    assert p.frame_stats is None
    pts, _ = H.defragile_points(h, H.cloud(1, h, pad), cen, R)
    ref_occ, ref = FR.mark(ORIGIN, h, n, pts, cen, R)
    assert p.set_point_cloud_filtered(ORIGIN, h, n, pts, q, pad) == ref == p.frame_stats
    assert np.array_equal(p._solver.field()[1], F.edt(ref_occ))
    cam, raw = H.image(M, 1, 64, 48, True, pad)
    depth, _ = H.defragile_image(h, cam, raw, cen, R)
    ref_occ2, ref2 = FR.mark_depth(ORIGIN, h, n, cam, depth, cen, R, occ=ref_occ)
    assert p.set_depth_image(ORIGIN, h, n, cam, depth, q, pad, keep=True) == ref2 == p.frame_stats
    assert np.array_equal(p._solver.field()[1], F.edt(ref_occ2))
    assert p.set_depth_image(ORIGIN, h, n, cam, depth)["n_robot"] == 0
    pad_c = H.pad_carve(h)
    cen_c, R_c = FR.filter_spheres(models, tables, q, pad_c)
    occ = FR.mark_depth(ORIGIN, h, n, cam, depth, np.zeros((0, 3)), np.zeros(0))[0]
    occ[FR.fragile_voxels(ORIGIN, h, occ, cen_c, R_c)] = 0
    ref_occ3, ref3 = FR.carve(ORIGIN, h, occ, cen_c, R_c)
    p.set_voxel_world(ORIGIN, h, occ)
    assert p.carve_robot(q, pad_c) == ref3 == p.frame_stats and ref3["n_cleared"] > 0
    assert np.array_equal(p._solver.field()[1], F.edt(ref_occ3))
    exe = str(tmp_path / "frame_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "frame_selftest.cpp"), "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert json.loads(lines[0])["host"]["order_wrong"] == 0
    rec = json.loads(lines[-1])
    assert rec["raw_status"] & 1 and rec["raw_t_first"] == 0.0 and rec["raw_d_min"] < 0.0
    assert rec["n_robot"] == rec["host_n_robot"] > 0 and rec["n_marked"] == rec["host_n_marked"] > 0 and rec["differ"] == 0
    assert rec["n_in"] == rec["n_robot"] + rec["n_marked"] and rec["filtered_t_first"] != 0.0 and rec["carved_t_first"] != 0.0 and rec["n_cleared"] > 0
    assert rec["depth_n_in"] == 48 * 36 == rec["depth_sum"] and rec["depth_n_invalid"] == 1
