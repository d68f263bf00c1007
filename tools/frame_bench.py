#!/usr/bin/env python3
"""Camera frames as voxel worlds (include/mpcmp_frame.h): what removing the robot from a frame costs.

1. mpcmp_set_field_points_filtered_device beside mpcmp_set_field_points_device on the same --points cloud and 256 x 256 x 128 grid (the cloud recipe
   of tools/field_bench.py, of which --robot-share is drawn on the robot's own shell instead), and beside mpcmp_set_field_device of the marked
   occupancy (a device copy and the three transform passes alone): the difference to it is marking plus filtering.
2. A 640 x 480 16-bit depth frame of a floor and the robot: mpcmp_set_field_depth_device (device events), and on a host clock mpcmp_set_field_depth
   (upload of the raw frame included) beside "unproject in NumPy, then mpcmp_set_field_points" (upload of 24 bytes per point included).
3. mpcmp_field_carve_device of a 128^3 grid with 5 % of its voxels occupied, beside mpcmp_set_field_device of the same grid (the rebuild alone).
Device events on a torch stream, --rounds rounds alternating all calls, medians; the first round is a warm-up and is dropped.  Prints one JSON line.
usage: frame_bench.py [--rounds 6] [--points 200000] [--robot-share 0.1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
BIG = ((-1.28, -1.28, -0.32), 0.01, (256, 256, 128))
CUBE = ((-1.28, -1.28, -0.32), 0.02, (128, 128, 128))
Q = np.array([0.3, -0.4, 0.2, -1.9, 0.1, 1.7, 0.4])


def shell_of(M, sph, pad, k, rng):
    cen = M.frame_spheres(M.default_model(), sph, Q, pad)
    s = rng.integers(cen.shape[0], size=k)
    d = rng.normal(size=(k, 3))
    return cen[s, :3] + cen[s, 3:4] * d / np.linalg.norm(d, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--robot-share", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    s = M.Solver(M.default_config(4, 1, margins=MARGINS), 4)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    rng = np.random.default_rng(3)
    origin, h, n = BIG
    pad = 4.34 * h + 0.02
    lo, ext = np.asarray(origin), h * np.asarray(n)
    n_rob = int(a.robot_share * a.points)
    k = (a.points - n_rob) // 4
    wall = lo + rng.random((k, 3)) * ext; wall[:, 0] = lo[0] + 0.9 * ext[0] + 0.01 * rng.random(k)
    floor = lo + rng.random((k, 3)) * ext; floor[:, 2] = lo[2] + 0.05 * ext[2] + 0.01 * rng.random(k)
    d = rng.normal(size=(k, 3)); ball = np.array([0.55, 0.0, 0.75]) + 0.15 * d / np.linalg.norm(d, axis=1, keepdims=True)
    m = a.points - n_rob - 3 * k
    rest = lo + rng.random((m, 3)) * ext; rest[:, 1] = lo[1] + 0.1 * ext[1] + 0.01 * rng.random(m)
    cloud = np.ascontiguousarray(np.concatenate([wall, floor, ball, rest, shell_of(M, sph, pad / 2, n_rob, rng)]))
    desc_big, desc_cube = M.field_desc(origin, h, n), M.field_desc(*CUBE)
    # a depth frame from above: the floor plane and the robot's spheres (r_s + pad / 2), by one z-buffer pass per sphere
    W, Hh = 640, 480
    Rc = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]]); tc = np.array([0.2, 0.0, 2.2])
    cam = M.camera(Rc, tc, 500.0, 500.0, (W - 1) / 2.0, (Hh - 1) / 2.0, W, Hh, depth_scale=0.001, z_min=0.2, z_max=3.0)
    v, u = np.divmod(np.arange(W * Hh), W)
    dc = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones(W * Hh)], axis=1) @ Rc.T
    z = (lo[2] + 0.05 * ext[2] - tc[2]) / dc[:, 2]
    for c in M.frame_spheres(M.default_model(), sph, Q, pad / 2):
        oc = tc - c[:3]
        A, Bq = (dc * dc).sum(axis=1), dc @ oc
        disc = Bq * Bq - A * (oc @ oc - c[3] ** 2)
        with np.errstate(invalid="ignore"):
            zs = (-Bq - np.sqrt(disc)) / A
        z = np.where((disc >= 0) & (zs > 0) & (zs < z), zs, z)
    depth = np.rint(z * 1000.0).astype(np.uint16).reshape(Hh, W)
    occ_cube = (rng.random(CUBE[2][::-1]) < 0.05).astype(np.uint8)
    pad_cube = 3.47 * CUBE[1] + 0.02
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tcloud = torch.from_numpy(cloud).cuda()
        tdepth = torch.from_numpy(depth.view(np.int16)).cuda()
        tcube = torch.from_numpy(occ_cube).cuda()
        tstats = torch.zeros(32, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream
    s.set_field_points(desc_big, cloud)
    occ_big = (s.field()[1] == 0).astype(np.uint8)
    with torch.cuda.stream(stream):
        tbig = torch.from_numpy(occ_big).cuda()
    stream.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    def stats():
        rec = np.frombuffer(tstats.cpu().numpy().tobytes(), dtype=M.FRAME_STATS_DTYPE)[0]
        return {k: int(rec[k]) for k in rec.dtype.names if k != "pad"}

    def host_ms(fn):
        t0 = time.perf_counter(); fn(); return 1e3 * (time.perf_counter() - t0)

    def numpy_unproject():
        zz = depth.reshape(-1).astype(np.float64) * 0.001
        ok = (depth.reshape(-1) != 0) & (zz >= cam["z_min"]) & (zz <= cam["z_max"])
        p = np.stack([zz * (u - cam["cx"]) / cam["fx"], zz * (v - cam["cy"]) / cam["fy"], zz], axis=1)[ok]
        s.set_field_points(desc_big, p @ Rc.T + tc)
    calls = {
        "points_plain": lambda: s.set_field_points_device(desc_big, a.points, tcloud.data_ptr(), stream=st),
        "points_filtered": lambda: s.set_field_points_filtered_device(desc_big, a.points, tcloud.data_ptr(), Q, pad, stats=tstats.data_ptr(), stream=st),
        "transform_only_256x256x128": lambda: s.set_field_device(desc_big, tbig.data_ptr(), stream=st),
        "depth_640x480_device": lambda: s.set_field_depth_device(desc_big, cam, tdepth.data_ptr(), M.DEPTH_U16, Q, pad, stats=tstats.data_ptr(), stream=st),
        "transform_only_128^3": lambda: s.set_field_device(desc_cube, tcube.data_ptr(), stream=st),
    }
    ms = {k: [] for k in list(calls) + ["carve_128^3", "depth_640x480_host_call", "numpy_unproject_then_set_field_points"]}
    seen = {}
    for rnd in range(a.rounds + 1):
        t = {}
        for k, fn in calls.items():
            t[k] = timed(fn)
            if k in ("points_filtered", "depth_640x480_device"):
                seen[k] = stats()
        t["carve_128^3"] = timed(lambda: s.field_carve_device(Q, pad_cube, stats=tstats.data_ptr(), stream=st))      # (the cube of the call before)
        seen["carve_128^3"] = stats()
        t["depth_640x480_host_call"] = host_ms(lambda: s.set_field_depth(desc_big, cam, depth, Q, pad))
        t["numpy_unproject_then_set_field_points"] = host_ms(numpy_unproject)
        if rnd:
            for k, x in t.items():
                ms[k].append(x)
    med = {k: round(float(np.median(x)), 4) for k, x in ms.items()}
    res = {"points": a.points, "robot_share": a.robot_share, "spheres": int(sph.shape[0]), "rounds": a.rounds, "ms_median": med,
           "ms_all": {k: [round(x, 4) for x in xs] for k, xs in ms.items()}, "counts": seen,
           "mark_and_filter_ms": round(med["points_filtered"] - med["transform_only_256x256x128"], 4),
           "mark_plain_ms": round(med["points_plain"] - med["transform_only_256x256x128"], 4),
           "carve_without_rebuild_ms": round(med["carve_128^3"] - med["transform_only_128^3"], 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
