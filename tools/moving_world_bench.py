#!/usr/bin/env python3
"""Clearance in a moving world beside its parts: device time of ONE mpcmp_start_delay_batch_device call of K delays against K
mpcmp_clearance_timed_batch_device calls on the same plans, and of the timed check against mpcmp_clearance_batch_device.

The plans, the robot and the world are those of tools/clearance_cert_bench.py (a seeded batch of scenarios.make_batch, B = 1,024, N = 13, solved
once; the skeleton spheres of link_spheres(0.06, 0.08); eight obstacles, two of each primitive; margin 0.02; n_pts = 200).  The first four obstacles
(one of each primitive) are tracked: 64 keys over 4 s, each drifting 0.3 m on a curve of its own.  Delays: K values from 0 to 2 s.
Device events around --reps back-to-back calls on a torch stream; --rounds rounds that alternate the contenders, after one warm-up round that is
dropped; medians reported.
Prints one JSON line.  usage: moving_world_bench.py [--B 1024] [--K 32] [--rounds 5] [--reps 10] [--n-pts 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clearance_cert_bench import MARGIN, MARGINS, world       # noqa: E402


def tracks(n_obs, n_key=64, span=4.0, seed=2):
    """the first four obstacles on tracks of their own: offsets [4][n_key][3] that drift 0.3 m along a seeded direction and wobble across it"""
    rng = np.random.default_rng(seed)
    fr = np.arange(n_key) / (n_key - 1)
    off = np.zeros((4, n_key, 3))
    for k in range(4):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        e = np.cross(d, (0.0, 0.0, 1.0)); e /= max(np.linalg.norm(e), 1e-9)
        off[k] = 0.3 * fr[:, None] * d + 0.05 * np.sin(2 * np.pi * fr)[:, None] * e
    track_of = np.full(n_obs, -1, dtype=np.int32)
    track_of[:4] = np.arange(4)
    return track_of, off, 0.0, span / (n_key - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n-pts", type=int, default=200)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, K, nseg = a.B, a.K, 4
    s = M.Solver(M.default_config(nseg, 20, margins=MARGINS), B)
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    s.set_robot_spheres(sph)
    obs = world(M)
    s.set_obstacles(obs)
    s.set_obstacle_tracks(*tracks(obs.shape[0]))
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    sx, su, sT, info = s.solve(x0, xf, s.warm_start_jerk(x0, xf, jmax))
    delays = np.linspace(0.0, 2.0, K)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dx, dT, dd = torch.from_numpy(sx).cuda(), torch.from_numpy(sT).cuda(), torch.from_numpy(delays).cuda()
        dts = [torch.full((B,), float(d), dtype=torch.float64, device="cuda") for d in delays]
        dclr = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dsd = torch.zeros(B * M.START_DELAY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dall = torch.zeros((B, K), dtype=torch.float64, device="cuda")
    st = stream.cuda_stream

    def search():
        s.start_delay_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, K, dd.data_ptr(), 0, a.n_pts, MARGIN, 0, dall.data_ptr(), dsd.data_ptr(), stream=st)

    def k_checks():
        for t in dts:
            s.clearance_timed_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, t.data_ptr(), a.n_pts, MARGIN, 0, dclr.data_ptr(), stream=st)

    def timed_check():
        s.clearance_timed_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, dts[0].data_ptr(), a.n_pts, MARGIN, 0, dclr.data_ptr(), stream=st)

    def static_check():
        s.clearance_device(B, dx.data_ptr(), dT.data_ptr(), a.n_pts, MARGIN, 0, dclr.data_ptr(), stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / a.reps

    contenders = {"start_delay": search, "k_timed_checks": k_checks, "timed": timed_check, "static": static_check}
    ms = {k: [] for k in contenders}
    for rnd in range(a.rounds + 1):
        t = {k: timed(fn) for k, fn in contenders.items()}
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    sd = np.frombuffer(dsd.cpu().numpy().tobytes(), dtype=M.START_DELAY_DTYPE)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"B": B, "N": s.N, "K": K, "spheres": int(sph.shape[0]), "obstacles": int(obs.shape[0]), "tracked": 4, "n_key": 64, "margin": MARGIN,
           "n_pts": a.n_pts, "rounds": a.rounds, "reps": a.reps,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "us_per_plan": {k: round(1e3 * v / B, 3) for k, v in med.items()},
           "k_checks_over_start_delay": round(med["k_timed_checks"] / med["start_delay"], 3), "timed_over_static": round(med["timed"] / med["static"], 3),
           "share": {"clear_at_0": round(float((sd["index"] == 0).mean()), 4), "waiting_helps": round(float((sd["index"] > 0).mean()), 4),
                     "no_clear_delay": round(float((sd["index"] < 0).mean()), 4)}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
