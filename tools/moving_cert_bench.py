#!/usr/bin/env python3
"""Certified clearance in a moving world beside its two parents: device time of mpcmp_clearance_certified_timed_batch_device (n_start = 4,
n_rest = 4, max_depth = 10, a wait and a hold of 0.5 s) in the moving world, of mpcmp_clearance_timed_batch_device at n_pts = 200 in the same
world, and of mpcmp_clearance_certified_batch_device in that world with its tracks removed; and, as the cost of the track phase and the rest logic
when they have nothing to do, of the new call in the world without tracks, without wait and hold, beside the static certificate.

The plans, the robot and the world are those of tools/moving_world_bench.py (a seeded batch of scenarios.make_batch, B = 1,024, N = 13, solved once;
the skeleton spheres of link_spheres(0.06, 0.08); eight obstacles, two of each primitive, the first four on tracks of 64 keys over 4 s; margin
0.02).  Two contexts hold the two worlds, so that no setter runs between the contenders.  Device events around --reps back-to-back calls on a torch
stream; --rounds rounds that alternate the contenders, after one warm-up round that is dropped; medians reported, and the n_eval distribution.
Prints one JSON line.  usage: moving_cert_bench.py [--B 1024] [--rounds 5] [--reps 20] [--n-start 4] [--n-rest 4] [--max-depth 10] [--n-pts 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clearance_cert_bench import MARGIN, MARGINS, world       # noqa: E402
from moving_world_bench import tracks                          # noqa: E402


def n_eval_stats(ne):
    ne = ne.astype(np.int64)
    return {"min": int(ne.min()), "median": float(np.median(ne)), "mean": round(float(ne.mean()), 1), "p90": float(np.percentile(ne, 90)),
            "max": int(ne.max()), "sum": int(ne.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-start", type=int, default=4)
    ap.add_argument("--n-rest", type=int, default=4)
    ap.add_argument("--max-depth", type=int, default=10)
    ap.add_argument("--n-pts", type=int, default=200)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, nseg = a.B, 4
    sph = M.link_spheres(M.default_model(), 0.06, 0.08)
    obs = world(M)
    moving, still = M.Solver(M.default_config(nseg, 20, margins=MARGINS), B), M.Solver(M.default_config(nseg, 1, margins=MARGINS), B)
    for s in (moving, still):
        s.set_robot_spheres(sph)
        s.set_obstacles(obs)
    moving.set_obstacle_tracks(*tracks(obs.shape[0]))
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    sx, su, sT, info = moving.solve(x0, xf, moving.warm_start_jerk(x0, xf, jmax))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dx, dT = torch.from_numpy(sx).cuda(), torch.from_numpy(sT).cuda()
        dts = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
        drest = torch.full((B,), 0.5, dtype=torch.float64, device="cuda")
        rec = {k: torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for k in ("mv", "timed", "static", "mv_static")}
        crt = {k: torch.zeros(B * M.CLEARANCE_CERT_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for k in ("mv", "static", "mv_static")}
    st = stream.cuda_stream
    contenders = {
        "certified_timed": lambda: moving.clearance_certified_timed_device(B, dx.data_ptr(), dT.data_ptr(), dts.data_ptr(), drest.data_ptr(), drest.data_ptr(),
                                                                           MARGIN, 0, a.n_start, a.n_rest, a.max_depth, rec["mv"].data_ptr(),
                                                                           crt["mv"].data_ptr(), stream=st),
        "timed": lambda: moving.clearance_timed_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, dts.data_ptr(), a.n_pts, MARGIN, 0, rec["timed"].data_ptr(),
                                                       stream=st),
        "certified_static": lambda: still.clearance_certified_device(B, dx.data_ptr(), dT.data_ptr(), MARGIN, 0, a.n_start, a.max_depth,
                                                                     rec["static"].data_ptr(), crt["static"].data_ptr(), stream=st),
        "certified_timed_in_static_world": lambda: still.clearance_certified_timed_device(B, dx.data_ptr(), dT.data_ptr(), 0, 0, 0, MARGIN, 0, a.n_start,
                                                                                          a.n_rest, a.max_depth, rec["mv_static"].data_ptr(),
                                                                                          crt["mv_static"].data_ptr(), stream=st),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / a.reps

    ms = {k: [] for k in contenders}
    for rnd in range(a.rounds + 1):
        t = {k: timed(fn) for k, fn in contenders.items()}
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    clr = {k: np.frombuffer(v.cpu().numpy().tobytes(), dtype=M.CLEARANCE_DTYPE) for k, v in rec.items()}
    cert = {k: np.frombuffer(v.cpu().numpy().tobytes(), dtype=M.CLEARANCE_CERT_DTYPE) for k, v in crt.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    share = lambda c: {"certified": round(float((c["status"] == 0).mean()), 4), "hit": round(float(((c["status"] & M.CLR_HIT) != 0).mean()), 4),       # noqa: E731
                       "undecided": round(float(((c["status"] & M.CLR_UNDECIDED) != 0).mean()), 4), "nan": round(float((c["status"] == M.CLR_NAN).mean()), 4)}
    res = {"B": B, "N": moving.N, "spheres": int(sph.shape[0]), "obstacles": int(obs.shape[0]), "tracked": 4, "n_key": 64, "margin": MARGIN,
           "n_start": a.n_start, "n_rest": a.n_rest, "max_depth": a.max_depth, "n_pts": a.n_pts, "wait": 0.5, "hold": 0.5, "rounds": a.rounds,
           "reps": a.reps, "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "us_per_plan": {k: round(1e3 * v / B, 3) for k, v in med.items()},
           "n_eval": {k: n_eval_stats(v["n_eval"]) for k, v in cert.items()},
           "ns_per_configuration": {"certified_timed": round(1e6 * med["certified_timed"] / max(int(cert["mv"]["n_eval"].sum()), 1), 2),
                                    "certified_static": round(1e6 * med["certified_static"] / max(int(cert["static"]["n_eval"].sum()), 1), 2),
                                    "timed": round(1e6 * med["timed"] / (B * (a.n_pts + 1)), 2)},
           "share": {k: share(v) for k, v in clr.items() if k != "timed"},
           "timed_share_hit": round(float((clr["timed"]["status"] == M.CLR_HIT).mean()), 4),
           "timed_clear_but_certified_hit": int(((clr["timed"]["status"] == 0) & ((clr["mv"]["status"] & M.CLR_HIT) != 0)).sum()),
           "static_world_records_equal": bool(np.array_equal(clr["static"]["status"], clr["mv_static"]["status"])
                                              and np.array_equal(cert["static"]["n_eval"], cert["mv_static"]["n_eval"])),
           "overhead_in_static_world": round(med["certified_timed_in_static_world"] / med["certified_static"], 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
