#!/usr/bin/env python3
"""Certified clearance beside the sampled check: device time of mpcmp_clearance_certified_batch_device at n_start = 4, max_depth = 10 and of
mpcmp_clearance_batch_device at n_pts = 200 on the same plans, and what the adaptive check did.

A seeded batch of scenarios.make_batch (B = 1,024, N = 13, 20 SQP iterations, jerk-limited warm start) is solved once; its solutions are checked
with the skeleton spheres of link_spheres(0.06, 0.08) in a world of eight obstacles (two of each primitive, seeded) at margin 0.02.  Device
events around --reps back-to-back calls on a torch stream; --rounds rounds that alternate the two checkers, after one warm-up round that is dropped;
medians reported.  Per evaluated configuration: the call's time over B x (n_pts + 1) for the sampled check and over the sum of n_eval for the
certified one.
Prints one JSON line.  usage: clearance_cert_bench.py [--B 1024] [--rounds 5] [--reps 20] [--n-start 4] [--max-depth 10] [--n-pts 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
MARGIN = 0.02


def world(M, seed=1):
    """eight obstacles, two of each primitive, in the arm's workspace; the first half-space is the floor"""
    rng = np.random.default_rng(seed)
    out = np.zeros(8, dtype=M.OBSTACLE_DTYPE)
    for i in range(8):
        kind = i % 4
        a = rng.uniform((-0.7, -0.7, 0.1), (0.7, 0.7, 1.0))
        if kind == M.OBS_SPHERE:
            out[i] = M.obstacle(kind, a, r=rng.uniform(0.03, 0.08))
        elif kind == M.OBS_CAPSULE:
            out[i] = M.obstacle(kind, a, a + rng.uniform(-0.3, 0.3, 3), rng.uniform(0.005, 0.03))
        elif kind == M.OBS_BOX:
            out[i] = M.obstacle(kind, a, rng.uniform(0.03, 0.10, 3), 0.0)
        elif i == 3:
            out[i] = M.obstacle(kind, (0.0, 0.0, 1.0), (-0.05, 0, 0))
        else:
            out[i] = M.obstacle(kind, (-1.0, 0.0, 0.0), (-0.9, 0, 0))          # a wall at x = 0.9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-start", type=int, default=4)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--n-pts", type=int, default=200)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, nseg = a.B, 4
    s = M.Solver(M.default_config(nseg, 20, margins=MARGINS), B)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    obs = world(M)
    s.set_obstacles(obs)
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    sx, su, sT, info = s.solve(x0, xf, s.warm_start_jerk(x0, xf, jmax))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dx, dT = torch.from_numpy(sx).cuda(), torch.from_numpy(sT).cuda()
        dclr = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dsam = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dcert = torch.zeros(B * M.CLEARANCE_CERT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream
    certified = lambda: s.clearance_certified_device(B, dx.data_ptr(), dT.data_ptr(), MARGIN, 0, a.n_start, a.max_depth, dclr.data_ptr(),       # noqa: E731
                                                     dcert.data_ptr(), stream=st)
    sampled = lambda: s.clearance_device(B, dx.data_ptr(), dT.data_ptr(), a.n_pts, MARGIN, 0, dsam.data_ptr(), stream=st)                   # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / a.reps

    ms = {"certified": [], "sampled": []}
    for rnd in range(a.rounds + 1):
        t = {"certified": timed(certified), "sampled": timed(sampled)}
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    clr = np.frombuffer(dclr.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)
    sam = np.frombuffer(dsam.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)
    cert = np.frombuffer(dcert.cpu().numpy().tobytes(), dtype=M.CLEARANCE_CERT_DTYPE)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ne = cert["n_eval"].astype(np.int64)
    res = {"B": B, "N": s.N, "spheres": int(sph.shape[0]), "obstacles": int(obs.shape[0]), "margin": MARGIN, "n_start": a.n_start,
           "max_depth": a.max_depth, "n_pts": a.n_pts, "rounds": a.rounds, "reps": a.reps,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "us_per_plan": {k: round(1e3 * v / B, 3) for k, v in med.items()},
           "n_eval": {"min": int(ne.min()), "median": float(np.median(ne)), "mean": round(float(ne.mean()), 1), "p90": float(np.percentile(ne, 90)),
                      "max": int(ne.max()), "sum": int(ne.sum())},
           "depth_max": int(cert["depth"].max()),
           "share": {"certified": round(float((clr["status"] == 0).mean()), 4), "hit": round(float(((clr["status"] & M.CLR_HIT) != 0).mean()), 4),
                     "undecided": round(float(((clr["status"] & M.CLR_UNDECIDED) != 0).mean()), 4),
                     "nan": round(float((clr["status"] == M.CLR_NAN).mean()), 4)},
           "sampled_share_hit": round(float((sam["status"] == M.CLR_HIT).mean()), 4),
           "sampled_clear_but_certified_hit": int(((sam["status"] == 0) & ((clr["status"] & M.CLR_HIT) != 0)).sum()),
           "ns_per_configuration": {"certified": round(1e6 * med["certified"] / max(int(ne.sum()), 1), 2),
                                    "sampled": round(1e6 * med["sampled"] / (B * (a.n_pts + 1)), 2)}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
