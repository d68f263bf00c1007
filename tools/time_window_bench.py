#!/usr/bin/env python3
"""Cost of per-problem final-time windows (mpcmp_set_time_windows) and of the time-synchronised solve (mpcmp_solve_batch_synced_device): the
headline configuration (1,024 problems, N = 13, 20 SQP) and the reference-as-shipped one (1,024 problems, N = 19, 2 SQP), each in four cases:
no rows; rows equal to [cfg.lbT, cfg.ubT] (the same problems: isolates the cost of the per-problem row reads); mixed rows (a third free, a third
at 1.2 x their free optimum fixed, a third in [1.1, 1.6] x it: other problems, other iteration counts); and a synchronised solve in 128 groups of
8 (no rows).  Timed the way bench.py times its batch workloads (device buffers, jerk-limited warm start + solve per step).  The cases of a
configuration run in alternation on one context, `--repeats` times, so that drift of the clock hits all alike (the rows are set or cleared
between two timed runs: a context per case shares the hardware queues with the others unevenly, and that alone made a later context 7 % slower
on the MI355X); printed: traj/s per case as median [min, max] over the repeats, the cost of the rows, and the synchronised solve's rate over
the plain one.
usage: time_window_bench.py [--steps K] [--warmup W] [--repeats R]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    dev = torch.device("cuda", 0)
    B = args.batch
    for name, nseg, sqp in (("headline", 4, 20), ("shipped", 6, 2)):
        N = 3 * nseg + 1
        x0_h, xf_h = scenarios.make_batch(B, MARGINS)
        x0, xf = torch.from_numpy(x0_h).to(dev), torch.from_numpy(xf_h).to(dev)
        bufs = [torch.zeros(B, N, 14, dtype=torch.float64, device=dev), torch.zeros(B, N, 7, dtype=torch.float64, device=dev),
                torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, N, 14, dtype=torch.float64, device=dev),
                torch.zeros(B, N, 7, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)]
        info = torch.zeros(B, 64, dtype=torch.uint8, device=dev)
        group = torch.from_numpy((np.arange(B) // 8 % 128).astype(np.int32)).to(dev)
        group_T = torch.zeros(128, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        jmax = MARGINS[4] * M.default_limits()["jmax"]
        cfg = M.default_config(nseg, sqp, margins=MARGINS)
        s = M.Solver(cfg, B)
        T_free = s.solve(x0_h, xf_h, s.warm_start_jerk(x0_h, xf_h, jmax))[2]
        kind = np.arange(B) % 3
        rows = {"none": None, "config": (np.full(B, cfg.lbT), np.full(B, cfg.ubT)),
                "mixed": (np.where(kind == 1, 1.2 * T_free, np.where(kind == 2, 1.1 * T_free, 0.0)),
                          np.where(kind == 1, 1.2 * T_free, np.where(kind == 2, 1.6 * T_free, 10.0))),
                "synced": None}
        wx, wu, wT, sx, su, sT = [b.data_ptr() for b in bufs]

        def select(c):
            if rows[c] is None:
                s.clear_time_windows()
            else:
                s.set_time_windows(*rows[c])

        def run(c, k):
            for _ in range(k):
                s.warm_start_jerk_device(B, x0.data_ptr(), xf.data_ptr(), jmax, wx, wu, wT, stream=stream)
                if c == "synced":
                    s.solve_synced_device(B, x0.data_ptr(), xf.data_ptr(), group.data_ptr(), 128, sx, su, sT, info.data_ptr(), group_T.data_ptr(),
                                          warm=(wx, wu, wT), stream=stream)
                else:
                    s.solve_device(B, x0.data_ptr(), xf.data_ptr(), sx, su, sT, info.data_ptr(), warm=(wx, wu, wT), stream=stream)
            torch.cuda.synchronize(dev)

        rates = {c: [] for c in rows}
        for c in rows:
            select(c)
            run(c, args.warmup)
        for _ in range(args.repeats):
            for c in rows:
                select(c)
                t0 = time.perf_counter()
                run(c, args.steps)
                rates[c].append(B * args.steps / (time.perf_counter() - t0))
        med = {c: float(np.median(r)) for c, r in rates.items()}
        for c, r in rates.items():
            print("%-8s N = %d, %d SQP, %-6s: %.0f traj/s  [%.0f, %.0f] over %d alternating repeats"
                  % (name, N, sqp, c, med[c], min(r), max(r), args.repeats))
        for c in ("config", "mixed"):
            print("%-8s time with %s rows against none: %+.2f %% (median against median)" % (name, c, 100.0 * (med["none"] / med[c] - 1.0)))
        print("%-8s synced (128 groups of 8) over plain: %.3f x the rate" % (name, med["synced"] / med["none"]))


if __name__ == "__main__":
    main()
