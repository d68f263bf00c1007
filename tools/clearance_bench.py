#!/usr/bin/env python3
"""Batched clearance checks: device time of mpcmp_clearance_batch_device beside the solve it follows.

The headline batch (B = 1,024, N = 13, 20 SQP iterations, jerk-limited warm start) is solved once; its solutions are then checked at n_pts + 1
samples with the skeleton spheres of link_spheres(0.06, 0.08) against 0, 64 (16 of each primitive) and 256 obstacles.  Device events around the
calls on a torch stream, --rounds alternating rounds of (solve, check at every obstacle count, traj_stats), medians reported; the first round is a
warm-up and is dropped.  mpcmp_traj_stats_batch, the parent's kernel that samples and runs a forward pass per sample, has only a host-pointer entry
point: its figure is a host clock around the call INCLUDING its copies, and the clearance call is timed the same way beside it.
Kernel against kernel (k_clearance beside k_traj_stats, without the copies) comes from a kernel trace of this tool, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/clearance_bench.py --rounds 2
and the per-kernel rows of OUT/*/*_kernel_stats.csv (k_clearance runs once per obstacle count and round, twice more for the host-pointer calls).
Distance evaluations per call, from the shapes: B x (n_pts + 1) x spheres x obstacles.
Prints one JSON line.  usage: clearance_bench.py [--B 1024] [--n-pts 200] [--rounds 4] [--obstacles 0 64 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


def obstacles(M, n, seed=1):
    """n obstacles, a quarter of each primitive, scattered through the arm's workspace"""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=M.OBSTACLE_DTYPE)
    for i in range(n):
        kind = i % 4
        a = rng.uniform((-0.8, -0.8, 0.0), (0.8, 0.8, 1.1))
        if kind == M.OBS_SPHERE:
            out[i] = M.obstacle(kind, a, r=rng.uniform(0.02, 0.08))
        elif kind == M.OBS_CAPSULE:
            out[i] = M.obstacle(kind, a, a + rng.uniform(-0.3, 0.3, 3), rng.uniform(0.02, 0.05))
        elif kind == M.OBS_BOX:
            out[i] = M.obstacle(kind, a, rng.uniform(0.03, 0.12, 3), 0.0)
        else:
            nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm)
            out[i] = M.obstacle(kind, nrm, (-rng.uniform(0.9, 1.3), 0, 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-pts", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--obstacles", type=int, nargs="+", default=[0, 64, 256])
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, n_pts, nseg = a.B, a.n_pts, 4
    cfg = M.default_config(nseg, 20, margins=MARGINS)
    s = M.Solver(cfg, B)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    N = s.N
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
        tx0, txf = torch.from_numpy(x0).cuda(), torch.from_numpy(xf).cuda()
        wx, wu, wT, sx, su, sT = d(B, N, 14), d(B, N, 7), d(B), d(B, N, 14), d(B, N, 7), d(B)
        tinfo = torch.zeros(B * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        tout = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream
    s.warm_start_jerk_device(B, tx0.data_ptr(), txf.data_ptr(), jmax, wx.data_ptr(), wu.data_ptr(), wT.data_ptr(), stream=st)
    worlds = {n: obstacles(M, n) for n in a.obstacles}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    ms = {"solve": [], "traj_stats_host_call": [], "clearance_host_call": []}
    ms.update({"clearance_%d" % n: [] for n in a.obstacles})
    hits = {}
    for rnd in range(a.rounds + 1):
        t = {"solve": timed(lambda: s.solve_device(B, tx0.data_ptr(), txf.data_ptr(), sx.data_ptr(), su.data_ptr(), sT.data_ptr(), tinfo.data_ptr(),
                                                   warm=(wx.data_ptr(), wu.data_ptr(), wT.data_ptr()), stream=st))}
        for n in a.obstacles:
            if n:
                s.set_obstacles(worlds[n])
            else:
                s.clear_obstacles()
            t["clearance_%d" % n] = timed(lambda: s.clearance_device(B, sx.data_ptr(), sT.data_ptr(), n_pts, 0.02, 0, tout.data_ptr(), stream=st))
            hits[n] = int((np.frombuffer(tout.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE)["status"] == M.CLR_HIT).sum())
        hx, hu, hT = sx.cpu().numpy(), su.cpu().numpy(), sT.cpu().numpy()
        t0 = time.perf_counter(); s.traj_stats(hx, hu, hT, xf, n_pts); t["traj_stats_host_call"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter(); s.clearance(hx, hT, n_pts, 0.02, 0); t["clearance_host_call"] = 1e3 * (time.perf_counter() - t0)
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"B": B, "N": N, "n_pts": n_pts, "spheres": int(sph.shape[0]), "rounds": a.rounds,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "problems_hit": hits,
           "host_call_obstacles": a.obstacles[-1]}
    for n in a.obstacles:
        c = med["clearance_%d" % n]
        res["clearance_%d" % n] = {"problems_per_s": round(B / (c * 1e-3)), "share_of_solve": round(c / med["solve"], 5),
                                   "distance_evals_per_s": round(B * (n_pts + 1) * sph.shape[0] * n / (c * 1e-3))}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
