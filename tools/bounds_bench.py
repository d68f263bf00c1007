#!/usr/bin/env python3
"""Cost of per-problem bounds (mpcmp_set_bounds): the headline configuration (1,024 problems, N = 13, 20 SQP) and the reference-as-shipped one
(1,024 problems, N = 19, 2 SQP), each in three cases: no rows; rows equal to the configuration's six tables (the same problems: isolates the
cost of the per-problem row reads); and the mixed table of tests/test_gpu_bounds.py (problem i of kind i % 6: default, slow, weak, narrow, floor,
and in place of `locked`, which needs its own states, a second slow row: other problems, other iteration counts, reported, not compared).
Timed the way bench.py times its batch workloads (device buffers, jerk-limited warm start + solve per step).  The cases of a configuration run
in alternation on one context, `--repeats` times, so that drift of the clock hits all alike (the rows are set or cleared between two timed runs);
printed: traj/s per case as median [min, max] over the repeats, the mean ADMM iterations per problem of each case, and the cost of the rows.
usage: bounds_bench.py [--steps K] [--warmup W] [--repeats R]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
MIXED = ((0.9, 0.9, 0.5, 0.9, 0.05), (0.9, 0.45, 0.25, 0.9, 0.05), (0.9, 0.9, 0.5, 0.5, 0.05), (0.8, 0.9, 0.5, 0.9, 0.05), (0.9, 0.9, 0.5, 0.9, 0.25),
         (0.9, 0.45, 0.25, 0.9, 0.05))


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
        info = torch.zeros(B * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        jmax = MARGINS[4] * M.default_limits()["jmax"]
        cfg = M.default_config(nseg, sqp, margins=MARGINS)
        s = M.Solver(cfg, B)
        mixed = np.zeros(B, dtype=M.BOUNDS_DTYPE)
        for i in range(B):
            mixed[i] = M.bounds_from_margins(*MIXED[i % 6])
        rows = {"none": None, "config": s.bounds_table(n=B), "mixed": mixed}
        wx, wu, wT, sx, su, sT = [b.data_ptr() for b in bufs]

        def select(c):
            if rows[c] is None:
                s.clear_bounds()
            else:
                s.set_bounds(rows[c])

        def run(c, k):
            for _ in range(k):
                s.warm_start_jerk_device(B, x0.data_ptr(), xf.data_ptr(), jmax, wx, wu, wT, stream=stream)
                s.solve_device(B, x0.data_ptr(), xf.data_ptr(), sx, su, sT, info.data_ptr(), warm=(wx, wu, wT), stream=stream)
            torch.cuda.synchronize(dev)

        rates = {c: [] for c in rows}
        iters = {}
        for c in rows:
            select(c)
            run(c, args.warmup)
            iters[c] = float(np.frombuffer(info.cpu().numpy().tobytes(), dtype=M.INFO_DTYPE)["qp_iters_total"].mean())
        for _ in range(args.repeats):
            for c in rows:
                select(c)
                t0 = time.perf_counter()
                run(c, args.steps)
                rates[c].append(B * args.steps / (time.perf_counter() - t0))
        med = {c: float(np.median(r)) for c, r in rates.items()}
        for c, r in rates.items():
            print("%-8s N = %d, %d SQP, %-6s: %.0f traj/s  [%.0f, %.0f] over %d alternating repeats, %.1f ADMM iterations per problem"
                  % (name, N, sqp, c, med[c], min(r), max(r), args.repeats, iters[c]))
        print("%-8s time with config rows against none: %+.2f %% (median against median; the same problems)" % (name, 100.0 * (med["none"] / med["config"] - 1.0)))
        print("%-8s time with mixed rows against none: %+.2f %% (other problems: reported, not a cost of the reads)" % (name, 100.0 * (med["none"] / med["mixed"] - 1.0)))


if __name__ == "__main__":
    main()
