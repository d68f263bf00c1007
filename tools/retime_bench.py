#!/usr/bin/env python3
"""Retiming: device time of mpcmp_retime_batch_device and of mpcmp_sample_retimed_batch_device beside the solve they follow and beside
mpcmp_limits_batch_device, and what retiming gains over the uniform stretch on a solved benchmark batch.

The headline batch (B = 1,024, N = 13, 20 SQP iterations, jerk-limited warm start) is solved once per round; its solutions are then checked
(mpcmp_limits_batch_device, n_pts = n_grid), retimed at n_grid + 1 grid points and the retimed plans sampled at n_grid + 1 times.  Device events
around the *_device calls on a torch stream, --rounds rounds, medians reported; the first round is a warm-up and is dropped.
Kernel against kernel (k_retime beside k_limits, the kernel that shares its coefficient work) comes from a kernel trace of this tool, in a run of
its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/retime_bench.py --rounds 2
and the k_retime / k_limits rows of OUT/*/*_kernel_stats.csv.
Reported over the plans with a clean solve status: the median and the largest T_new / T of the feasible ones beside the median and the largest
stretch, and the share reported infeasible; with a NULL spec (the joint limits alone) and with the reference benchmark's tool limits 1.7 m/s and
2.5 rad/s.  The retimed groups are those a stretch cures too (QD, QDD, TOOL_LIN, TOOL_ANG) for the comparison, and all groups for the shares.
Prints one JSON line.  usage: retime_bench.py [--B 1024] [--n-grid 200] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-grid", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, n, nseg = a.B, a.n_grid, 4
    s = M.Solver(M.default_config(nseg, 20, margins=MARGINS), B)
    x0, xf = scenarios.make_batch(B, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    N = s.N
    kinematic = (1 << M.LIM_QD) | (1 << M.LIM_QDD) | (1 << M.LIM_TOOL_LIN) | (1 << M.LIM_TOOL_ANG)
    tool = M.retime_spec(1.7, 2.5)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
        tx0, txf = torch.from_numpy(x0).cuda(), torch.from_numpy(xf).cuda()
        wx, wu, wT, sx, su, sT = d(B, N, 14), d(B, N, 7), d(B), d(B, N, 14), d(B, N, 7), d(B)
        prof, rows = d(B, n + 1, 2), d(B, n + 1, 29)
        tinfo = torch.zeros(B * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        tlim = torch.zeros(B * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        trec = torch.zeros(B * M.RETIME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = stream.cuda_stream
    s.warm_start_jerk_device(B, tx0.data_ptr(), txf.data_ptr(), jmax, wx.data_ptr(), wu.data_ptr(), wT.data_ptr(), stream=st)
    traj = (sx.data_ptr(), su.data_ptr(), sT.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    ms = {"solve": [], "limits": [], "retime": [], "sample_retimed": []}
    for rnd in range(a.rounds + 1):
        t = {"solve": timed(lambda: s.solve_device(B, tx0.data_ptr(), txf.data_ptr(), *traj, tinfo.data_ptr(),
                                                   warm=(wx.data_ptr(), wu.data_ptr(), wT.data_ptr()), stream=st)),
             "limits": timed(lambda: s.limits_device(B, *traj, n, tlim.data_ptr(), M.limits_spec(0.0, 1.7, 2.5), stream=st)),
             "retime": timed(lambda: s.retime_device(B, *traj, n, prof.data_ptr(), trec.data_ptr(), tool, stream=st)),
             "sample_retimed": timed(lambda: s.sample_retimed_device(B, *traj, n, prof.data_ptr(), n, rows.data_ptr(), stream=st))}
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    info = np.frombuffer(tinfo.cpu().numpy().tobytes(), dtype=M.INFO_DTYPE)
    ok = (info["status"] & (M.STATUS_HARD | M.STATUS_OUTSIDE_TOL | M.STATUS_T_OUT_OF_BOX)) == 0
    T = sT.cpu().numpy()

    def records(spec, lim_spec):
        s.retime_device(B, *traj, n, prof.data_ptr(), trec.data_ptr(), spec, stream=st)
        s.limits_device(B, *traj, n, tlim.data_ptr(), lim_spec, stream=st)
        stream.synchronize()
        return (np.frombuffer(trec.cpu().numpy().tobytes(), dtype=M.RETIME_DTYPE).copy(),
                np.frombuffer(tlim.cpu().numpy().tobytes(), dtype=M.LIMITS_DTYPE).copy())

    def gain(lin, ang):
        rec, lim = records(M.retime_spec(lin, ang, 1.0, kinematic), M.limits_spec(0.0, lin, ang))
        good = ok & (rec["status"] == 0) & np.isfinite(lim["stretch"])
        if not good.any():
            return {}
        r = rec["T_new"][good] / T[good]
        return {"plans": int(good.sum()), "T_new_over_T_median": float(np.median(r)), "T_new_over_T_max": float(r.max()),
                "stretch_median": float(np.median(lim["stretch"][good])), "stretch_max": float(lim["stretch"][good].max()),
                "rate_min_median": float(np.median(rec["rate_min"][good]))}

    def infeasible(spec):
        rec, _ = records(spec, None)
        return round(float(((rec["status"][ok] & M.RT_INFEASIBLE) != 0).mean()), 4) if ok.any() else None

    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"B": B, "N": N, "n_grid": n, "rounds": a.rounds, "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "retime": {"problems_per_s": round(B / (med["retime"] * 1e-3)), "share_of_solve": round(med["retime"] / med["solve"], 5),
                      "over_limits": round(med["retime"] / med["limits"], 2)},
           "plans_clean": int(ok.sum()),
           "joint_limits": gain(np.inf, np.inf), "with_tool_limits": gain(1.7, 2.5),
           "share_infeasible": {"null_spec": infeasible(None), "with_tool_limits": infeasible(tool)}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
