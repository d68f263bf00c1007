#!/usr/bin/env python3
"""Voxel worlds: device time of building a distance field from a point cloud, and of the field check beside the primitive check.

1. mpcmp_set_field_points_device (zero the occupancy, mark the points, three transform passes) from --points seeded points spread through the
   grid, at 128^3 and 256 x 256 x 128, beside scipy.ndimage.distance_transform_edt of the same occupancy on the CPU (one run, a host clock).
2. mpcmp_clearance_field_batch_device at B plans, n_pts + 1 samples and the 24 skeleton spheres of link_spheres(0.06, 0.08) against the 128^3 field,
   beside mpcmp_clearance_batch_device with 64 obstacles (16 of each primitive) on the same plans.  The plans are the jerk-limited moves of the
   headline batch (no solve is needed to time a check).
Device events around the calls on a torch stream, --rounds warm rounds alternating all calls, medians reported; the first round is a warm-up and is
dropped.  Min-plus steps per build, from the shapes: voxels x (n0 + n1 + n2); gathers per check: B x (n_pts + 1) x spheres.  Kernel against
kernel comes from a kernel trace of this tool, in a run of its own:  rocprofv3 --kernel-trace --stats -d OUT -- python tools/field_bench.py --rounds 2
Prints one JSON line.  usage: field_bench.py [--B 1024] [--n-pts 200] [--rounds 6] [--points 200000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
GRIDS = {"128x128x128": ((-1.28, -1.28, -0.32), 0.02, (128, 128, 128)), "256x256x128": ((-1.28, -1.28, -0.32), 0.01, (256, 256, 128))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-pts", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--points", type=int, default=200000)
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    from clearance_bench import obstacles
    B, n_pts, nseg = a.B, a.n_pts, 4
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    s.set_obstacles(obstacles(M, 64))
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    N = s.N
    rng = np.random.default_rng(3)
    clouds, descs = {}, {}
    for name, (origin, h, n) in GRIDS.items():
        # a cloud as a camera leaves it: points on a few surfaces (planes and a sphere shell) away from the robot's base, not a uniform fog
        lo, ext = np.asarray(origin), h * np.asarray(n)
        k = a.points // 4
        wall = lo + rng.random((k, 3)) * ext; wall[:, 0] = lo[0] + 0.9 * ext[0] + 0.01 * rng.random(k)
        floor = lo + rng.random((k, 3)) * ext; floor[:, 2] = lo[2] + 0.05 * ext[2] + 0.01 * rng.random(k)
        d = rng.normal(size=(k, 3)); shell = np.array([0.55, 0.0, 0.75]) + 0.15 * d / np.linalg.norm(d, axis=1, keepdims=True)
        rest = lo + rng.random((a.points - 3 * k, 3)) * ext; rest[:, 1] = lo[1] + 0.1 * ext[1] + 0.01 * rng.random(a.points - 3 * k)
        clouds[name] = np.ascontiguousarray(np.concatenate([wall, floor, shell, rest]))
        descs[name] = M.field_desc(origin, h, n)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
        tx0, txf = torch.from_numpy(x0).cuda(), torch.from_numpy(xf).cuda()
        wx, wu, wT = d(B, N, 14), d(B, N, 7), d(B)
        tout = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        tpts = {k: torch.from_numpy(v).cuda() for k, v in clouds.items()}
    st = stream.cuda_stream
    s.warm_start_jerk_device(B, tx0.data_ptr(), txf.data_ptr(), jmax, wx.data_ptr(), wu.data_ptr(), wT.data_ptr(), stream=st)
    stream.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    def records():
        return np.frombuffer(tout.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)

    check_grid = "128x128x128"
    ms = {"build_" + k: [] for k in GRIDS}
    ms.update({"clearance_field": [], "clearance_64_obstacles": []})
    hits = {}
    for rnd in range(a.rounds + 1):
        t = {}
        for name in ("256x256x128", check_grid):                      # (the check's grid last: it stays in force)
            t["build_" + name] = timed(lambda: s.set_field_points_device(descs[name], a.points, tpts[name].data_ptr(), stream=st))
        t["clearance_field"] = timed(lambda: s.clearance_field_device(B, wx.data_ptr(), wT.data_ptr(), n_pts, 0.02, tout.data_ptr(), stream=st))
        hits["field"] = int((records()["status"] == M.CLR_HIT).sum())
        t["clearance_64_obstacles"] = timed(lambda: s.clearance_device(B, wx.data_ptr(), wT.data_ptr(), n_pts, 0.02, 0, tout.data_ptr(), stream=st))
        hits["obstacles"] = int((records()["status"] == M.CLR_HIT).sum())
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"B": B, "N": N, "n_pts": n_pts, "spheres": int(sph.shape[0]), "points": a.points, "rounds": a.rounds, "check_grid": check_grid,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "problems_hit": hits}
    for name, (origin, h, n) in GRIDS.items():
        s.set_field_points(descs[name], clouds[name])
        d2 = s.field()[1]
        occ = d2 == 0
        t0 = time.perf_counter(); ref = ndimage.distance_transform_edt(~occ); cpu_ms = 1e3 * (time.perf_counter() - t0)
        steps = int(np.prod(n)) * int(np.sum(n))
        res[name] = {"occupied": int(occ.sum()), "scipy_edt_ms": round(cpu_ms, 1), "same_as_scipy": bool(np.array_equal(np.rint(ref ** 2).astype(np.uint32), d2)),
                     "minplus_steps": steps, "minplus_steps_per_s": round(steps / (med["build_" + name] * 1e-3))}
    g = B * (n_pts + 1) * int(sph.shape[0])
    res["gathers"] = g
    res["gathers_per_s"] = round(g / (med["clearance_field"] * 1e-3))
    res["distance_evals_per_s_64_obstacles"] = round(g * 64 / (med["clearance_64_obstacles"] * 1e-3))
    res["field_over_primitive_time"] = round(med["clearance_field"] / med["clearance_64_obstacles"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
