#!/usr/bin/env python3
"""Between-node limit checks: device time of mpcmp_limits_batch_device beside the solve it follows and beside mpcmp_traj_stats_batch, and how often
the plans of a solved benchmark batch leave their bounds between the nodes.

The headline batch (B = 1,024, N = 13, 20 SQP iterations, jerk-limited warm start) is solved once per round; its solutions are then checked at
n_pts + 1 samples (tol 1e-6, the reference benchmark's tool speed limits 1.7 m/s and 2.5 rad/s).  Device events around the *_device calls on a torch
stream, --rounds alternating rounds of (solve, check), medians reported; the first round is a warm-up and is dropped.
mpcmp_traj_stats_batch, the parent's kernel that does the same per-sample work (interpolation, RNEA, one forward-kinematics pass) and keeps every
sample in LDS, has only a host-pointer entry point: its figure here is a host clock around the call INCLUDING its copies, and the limits call is
timed the same way beside it.  Kernel against kernel (k_limits beside k_traj_stats, without the copies) comes from a kernel trace of this tool, in
a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/limits_bench.py --rounds 2
and the k_limits / k_traj_stats rows of OUT/*/*_kernel_stats.csv.
Violation shares: over the plans with a clean solve status, the share whose record has the bit of each group set, the median and the largest
excess per group, and the median and the largest stretch: with the tool limits, and for the joint limits alone (a NULL spec).
Prints one JSON line.  usage: limits_bench.py [--B 1024] [--n-pts 200] [--rounds 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
NAMES = ("Q", "QD", "QDD", "TAU", "HEIGHT", "TOOL_LIN", "TOOL_ANG")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-pts", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, n_pts, nseg = a.B, a.n_pts, 4
    s = M.Solver(M.default_config(nseg, 20, margins=MARGINS), B)
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    N = s.N
    spec = M.limits_spec(1e-6, 1.7, 2.5)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
        tx0, txf = torch.from_numpy(x0).cuda(), torch.from_numpy(xf).cuda()
        wx, wu, wT, sx, su, sT = d(B, N, 14), d(B, N, 7), d(B), d(B, N, 14), d(B, N, 7), d(B)
        tinfo = torch.zeros(B * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        tout = torch.zeros(B * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream
    s.warm_start_jerk_device(B, tx0.data_ptr(), txf.data_ptr(), jmax, wx.data_ptr(), wu.data_ptr(), wT.data_ptr(), stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    ms = {"solve": [], "limits": [], "traj_stats_host_call": [], "limits_host_call": []}
    for rnd in range(a.rounds + 1):
        t = {"solve": timed(lambda: s.solve_device(B, tx0.data_ptr(), txf.data_ptr(), sx.data_ptr(), su.data_ptr(), sT.data_ptr(), tinfo.data_ptr(),
                                                   warm=(wx.data_ptr(), wu.data_ptr(), wT.data_ptr()), stream=st)),
             "limits": timed(lambda: s.limits_device(B, sx.data_ptr(), su.data_ptr(), sT.data_ptr(), n_pts, tout.data_ptr(), spec, stream=st))}
        hx, hu, hT = sx.cpu().numpy(), su.cpu().numpy(), sT.cpu().numpy()
        t0 = time.perf_counter(); s.traj_stats(hx, hu, hT, xf, n_pts); t["traj_stats_host_call"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter(); s.limits(hx, hu, hT, n_pts, 1e-6, 1.7, 2.5); t["limits_host_call"] = 1e3 * (time.perf_counter() - t0)
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    lim = np.frombuffer(tout.cpu().numpy().tobytes(), dtype=M.LIMITS_DTYPE)
    s.limits_device(B, sx.data_ptr(), su.data_ptr(), sT.data_ptr(), n_pts, tout.data_ptr(), None, stream=st)
    stream.synchronize()
    joint = np.frombuffer(tout.cpu().numpy().tobytes(), dtype=M.LIMITS_DTYPE)
    info = np.frombuffer(tinfo.cpu().numpy().tobytes(), dtype=M.INFO_DTYPE)
    ok = (info["status"] & (M.STATUS_HARD | M.STATUS_OUTSIDE_TOL | M.STATUS_T_OUT_OF_BOX)) == 0
    ok &= (lim["status"] & M.LIM_NAN) == 0
    L = lim[ok]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"B": B, "N": N, "n_pts": n_pts, "rounds": a.rounds, "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "limits": {"problems_per_s": round(B / (med["limits"] * 1e-3)), "samples_per_s": round(B * (n_pts + 1) / (med["limits"] * 1e-3)),
                      "share_of_solve": round(med["limits"] / med["solve"], 5)},
           "plans_checked": int(ok.sum()),
           "share_over": {NAMES[g]: round(float(((L["status"] >> g) & 1).mean()), 4) for g in range(7)} if L.size else {},
           "excess_median": {NAMES[g]: float(np.median(L["excess"][:, g])) for g in range(7)} if L.size else {},
           "excess_max": {NAMES[g]: float(L["excess"][:, g].max()) for g in range(7)} if L.size else {},
           "stretch_median": float(np.median(L["stretch"])) if L.size else None, "stretch_max": float(L["stretch"].max()) if L.size else None,
           "stretch_joint_limits_median": float(np.median(joint[ok]["stretch"])) if L.size else None,
           "stretch_joint_limits_max": float(joint[ok]["stretch"].max()) if L.size else None}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
