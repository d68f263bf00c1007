#!/usr/bin/env python3
"""Batched tool-pose targets: device time of mpcmp_pose_targets_batch_device against the host loop over mpcmp_inverse_kinematics.

For B in {1024, 4096} and S in {1, 8, 16}: poses from forward kinematics of seeded in-bounds configurations (scenarios.sample_states),
starts from scenarios.ik_seeds, q_ref = None, twist = None.  Device: HIP events around the launch on a torch stream, best of --reps after
one warm-up launch.  Host: one thread, every (problem, start) through mpcmp_inverse_kinematics (what the kernel runs per lane), timed with
a host clock; --host-max P times only the first P problems and scales (reported as such).  Prints one JSON line per shape with the
fraction of problems whose chosen start qualifies (converged, inside the position bounds).
usage: ik_bench.py [--B 1024 4096] [--S 1 8 16] [--reps 5] [--host-max P]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--S", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=0, help="time the host loop on at most this many problems (0 = all)")
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    cfg = M.default_config(4, 3, margins=MARGINS)
    model = M.default_model()
    L = M.lib()
    s = M.Solver(cfg, 1)
    stream = torch.cuda.Stream()
    for B in a.B:
        q = scenarios.sample_states(B, MARGINS, stream_offset=10_000)[:, :7]
        R = np.zeros((B, 9)); p = np.zeros((B, 3))
        for b in range(B):
            _, p[b], Rb = M.tool_jacobian(model, q[b]); R[b] = Rb.ravel()
        for S in a.S:
            seeds = scenarios.ik_seeds(B, S, cfg)
            with torch.cuda.stream(stream):
                tR, tp, ts = [torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for v in (R, p, seeds)]
                txf = torch.zeros((B, 14), dtype=torch.float64, device="cuda")
                tinfo = torch.zeros((B, M.IK_INFO_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            ms = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                s.pose_targets_device(B, 0, tR.data_ptr(), tp.data_ptr(), 0, S, ts.data_ptr(), 0, txf.data_ptr(), tinfo.data_ptr(),
                                      stream=stream.cuda_stream)
                e1.record(stream)
                stream.synchronize()
                if rep:
                    ms.append(e0.elapsed_time(e1))
            info = np.frombuffer(tinfo.cpu().numpy().tobytes(), dtype=M.IK_INFO_DTYPE)
            qual = float(np.mean((info["status"] & (M.IK_NOT_CONVERGED | M.IK_Q_OUT_OF_BOUNDS)) == 0))
            nh = B if a.host_max <= 0 else min(B, a.host_max)
            qo = np.zeros(7); it = C.c_int(0); iters = 0
            Rh, ph, sh = [np.ascontiguousarray(v) for v in (R, p, seeds)]
            dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
            t0 = time.perf_counter()
            for b in range(nh):
                for k in range(S):
                    L.mpcmp_inverse_kinematics(C.byref(model), dp(Rh[b]), dp(ph[b]), dp(sh[b, k]), dp(qo), C.byref(it))
                    iters += it.value
            host_s = (time.perf_counter() - t0) * B / nh
            dev_ms = min(ms)
            print(json.dumps({"B": B, "S": S, "device_ms": round(dev_ms, 4), "device_ms_median": round(float(np.median(ms)), 4),
                              "host_s_one_thread": round(host_s, 3), "host_problems_timed": nh, "speedup": round(1e3 * host_s / dev_ms, 1),
                              "host_mean_iters": round(iters / (nh * S), 1), "device_max_iters_chosen": int(info["iters"].max()),
                              "qualifying_fraction": round(qual, 4)}), flush=True)


if __name__ == "__main__":
    main()
