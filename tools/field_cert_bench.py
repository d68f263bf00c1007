#!/usr/bin/env python3
"""Certified clearance against a voxel world beside its two neighbours, same plans, same run: device time of
  certified_field   mpcmp_clearance_certified_field_batch_device (k_clearance_cert_field) at n_start = 4, max_depth = 10 on a 128^3 field,
  sampled_field     mpcmp_clearance_field_batch_device (k_clearance_field) at n_pts = 200 on the same field,
  certified         mpcmp_clearance_certified_batch_device (k_clearance_cert) on the four primitives the field was rasterised from,
per batch of B = 1,024 plans and per evaluated interval (the call's time over the sum of n_eval; per sample for the sampled check).

The plans are the jerk-limited moves of the headline batch (no solve is needed to time a check), the robot the 24 skeleton spheres of
link_spheres(0.06, 0.08), the world one of each primitive (a sphere, a capsule, a box, the floor), the field its rasterisation on a grid of 2 cm
voxels (a voxel is occupied if its centre is within half a diagonal of a solid), margin 0.02.  Device events around --reps back-to-back calls on a
torch stream; --rounds rounds that alternate the three checkers, after one warm-up round that is dropped; medians reported.
--lib PATH times another build of the library (how the chunk of k_clearance_cert_field was chosen).
Prints one JSON line.  usage: field_cert_bench.py [--B 1024] [--rounds 5] [--reps 20] [--n-start 4] [--max-depth 10] [--n-pts 200] [--lib PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
MARGIN = 0.02
ORIGIN, H, N_GRID = (-1.28, -1.28, -0.32), 0.02, (128, 128, 128)


def world(M):
    return np.array([M.obstacle(M.OBS_SPHERE, (0.55, 0.0, 0.75), (0, 0, 0), 0.10), M.obstacle(M.OBS_BOX, (0.6, -0.5, 0.15), (0.1, 0.1, 0.15), 0.01),
                     M.obstacle(M.OBS_CAPSULE, (-0.5, 0.5, 0.2), (-0.5, 0.5, 1.0), 0.04),
                     M.obstacle(M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (-0.05, 0, 0), 0.0)], dtype=M.OBSTACLE_DTYPE)


def rasterise(M, obs):
    """occupancy [n2][n1][n0]: the voxels whose centre lies within h sqrt(3) / 2 of a solid (the signed distances of include/mpcmp.h)"""
    k, j, i = np.meshgrid(np.arange(N_GRID[2]), np.arange(N_GRID[1]), np.arange(N_GRID[0]), indexing="ij")
    c = np.asarray(ORIGIN) + H * (np.stack([i, j, k], axis=-1) + 0.5)
    occ = np.zeros(c.shape[:3], dtype=bool)
    for ob in obs:
        a, b, r = np.asarray(ob["a"], float), np.asarray(ob["b"], float), float(ob["r"])
        if ob["type"] == M.OBS_SPHERE:
            d = np.linalg.norm(c - a, axis=-1) - r
        elif ob["type"] == M.OBS_CAPSULE:
            e = b - a
            t = np.clip((c - a) @ e / (e @ e), 0.0, 1.0)
            d = np.linalg.norm(c - a - t[..., None] * e, axis=-1) - r
        elif ob["type"] == M.OBS_BOX:
            q = np.abs(c - a) - b
            d = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0) - r
        else:
            d = c @ a - b[0]
        occ |= d <= H * np.sqrt(3.0) / 2.0
    return occ.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-start", type=int, default=4)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--n-pts", type=int, default=200)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        import mpc_motion_planner_amd.capi as capi
        capi._SO = os.path.abspath(a.lib)
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, nseg = a.B, 4
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    obs = world(M)
    s.set_obstacles(obs)
    occ = rasterise(M, obs)
    s.set_field(M.field_desc(ORIGIN, H, N_GRID), occ)
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    N = s.N
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tx0, txf = torch.from_numpy(x0).cuda(), torch.from_numpy(xf).cuda()
        dx, du, dT = (torch.zeros(shape, dtype=torch.float64, device="cuda") for shape in ((B, N, 14), (B, N, 7), (B,)))
        rec = {k: torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for k in ("certified_field", "sampled_field", "certified")}
        crt = {k: torch.zeros(B * M.CLEARANCE_CERT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for k in ("certified_field", "certified")}
    st = stream.cuda_stream
    s.warm_start_jerk_device(B, tx0.data_ptr(), txf.data_ptr(), jmax, dx.data_ptr(), du.data_ptr(), dT.data_ptr(), stream=st)
    stream.synchronize()
    calls = {
        "certified_field": lambda: s.clearance_certified_field_device(B, dx.data_ptr(), dT.data_ptr(), MARGIN, a.n_start, a.max_depth,
                                                                      rec["certified_field"].data_ptr(), crt["certified_field"].data_ptr(), stream=st),
        "sampled_field": lambda: s.clearance_field_device(B, dx.data_ptr(), dT.data_ptr(), a.n_pts, MARGIN, rec["sampled_field"].data_ptr(), stream=st),
        "certified": lambda: s.clearance_certified_device(B, dx.data_ptr(), dT.data_ptr(), MARGIN, 0, a.n_start, a.max_depth, rec["certified"].data_ptr(),
                                                          crt["certified"].data_ptr(), stream=st),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / a.reps

    ms = {k: [] for k in calls}
    for rnd in range(a.rounds + 1):
        t = {k: timed(fn) for k, fn in calls.items()}
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    clr = {k: np.frombuffer(v.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE) for k, v in rec.items()}
    cert = {k: np.frombuffer(v.cpu().numpy().tobytes(), dtype=M.CLEARANCE_CERT_DTYPE) for k, v in crt.items()}
    work = {"certified_field": int(cert["certified_field"]["n_eval"].astype(np.int64).sum()), "sampled_field": B * (a.n_pts + 1),
            "certified": int(cert["certified"]["n_eval"].astype(np.int64).sum())}

    def share(c):
        return {"clear": round(float((c["status"] == 0).mean()), 4), "hit": round(float(((c["status"] & M.CLR_HIT) != 0).mean()), 4),
                "undecided": round(float(((c["status"] & M.CLR_UNDECIDED) != 0).mean()), 4)}
    res = {"lib": a.lib or "default", "B": B, "N": N, "spheres": int(sph.shape[0]), "grid": list(N_GRID), "h": H, "occupied": int(occ.sum()),
           "margin": MARGIN, "n_start": a.n_start, "max_depth": a.max_depth, "n_pts": a.n_pts, "rounds": a.rounds, "reps": a.reps,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "evaluations": work, "ns_per_evaluation": {k: round(1e6 * med[k] / max(work[k], 1), 2) for k in med},
           "depth_max": {k: int(v["depth"].max()) for k, v in cert.items()},
           "n_eval_max": {k: int(v["n_eval"].max()) for k, v in cert.items()},
           "share": {k: share(v) for k, v in clr.items()},
           "sampled_clear_but_certified_hit": int(((clr["sampled_field"]["status"] == 0) & ((clr["certified_field"]["status"] & M.CLR_HIT) != 0)).sum())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
