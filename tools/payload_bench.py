#!/usr/bin/env python3
"""Cost of per-problem payloads (mpcmp_set_payloads): the headline configuration (1,024 problems, N = 13, 20 SQP) and the reference-as-shipped
one (1,024 problems, N = 19, 2 SQP), each without payload rows, with a table of zero payloads (the same problems: isolates the cost of the
per-problem model reads) and with a mixed table (0 / 0.5 / 2 / 3 kg, off-axis COM, full inertia: other problems, other iteration counts), timed
the way bench.py times its batch workloads (device buffers, jerk-limited warm start + solve per step).  The cases of a configuration run in
alternation, `--repeats` times, so that drift of the clock hits both alike; printed: traj/s per case as median [min, max] over the repeats and
the relative cost of the table.  usage: payload_bench.py [--steps K] [--warmup W] [--repeats R]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
I_FULL = np.array([[2.1e-3, 3.0e-4, -1.5e-4], [3.0e-4, 1.7e-3, 2.5e-4], [-1.5e-4, 2.5e-4, 2.6e-3]])
PAYLOADS = [(0.0, (0.0, 0.0, 0.257), 0.0 * I_FULL), (0.5, (0.012, -0.021, 0.287), 0.25 * I_FULL),
            (2.0, (-0.015, 0.01, 0.30), I_FULL), (3.0, (0.02, 0.015, 0.31), 1.5 * I_FULL)]


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
    kinds = np.random.default_rng(0).permutation(np.arange(B) % len(PAYLOADS))
    table = (np.array([PAYLOADS[k][0] for k in kinds]), np.array([PAYLOADS[k][1] for k in kinds]), np.array([PAYLOADS[k][2] for k in kinds]))
    for name, nseg, sqp in (("headline", 4, 20), ("shipped", 6, 2)):
        N = 3 * nseg + 1
        x0_h, xf_h = scenarios.make_batch(B, MARGINS)
        x0, xf = torch.from_numpy(x0_h).to(dev), torch.from_numpy(xf_h).to(dev)
        bufs = [torch.zeros(B, N, 14, dtype=torch.float64, device=dev), torch.zeros(B, N, 7, dtype=torch.float64, device=dev),
                torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, N, 14, dtype=torch.float64, device=dev),
                torch.zeros(B, N, 7, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)]
        info = torch.zeros(B, 64, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        jmax = MARGINS[4] * M.default_limits()["jmax"]
        cfg = M.default_config(nseg, sqp, margins=MARGINS)
        solvers = {"none": M.Solver(cfg, B), "zeros": M.Solver(cfg, B), "mixed": M.Solver(cfg, B)}
        solvers["zeros"].set_payloads(np.zeros(B))
        solvers["mixed"].set_payloads(*table)
        wx, wu, wT, sx, su, sT = [b.data_ptr() for b in bufs]

        def run(s, k):
            for _ in range(k):
                s.warm_start_jerk_device(B, x0.data_ptr(), xf.data_ptr(), jmax, wx, wu, wT, stream=stream)
                s.solve_device(B, x0.data_ptr(), xf.data_ptr(), sx, su, sT, info.data_ptr(), warm=(wx, wu, wT), stream=stream)
            torch.cuda.synchronize(dev)

        rates = {c: [] for c in solvers}
        for c, s in solvers.items():
            run(s, args.warmup)
        for _ in range(args.repeats):
            for c, s in solvers.items():
                t0 = time.perf_counter()
                run(s, args.steps)
                rates[c].append(B * args.steps / (time.perf_counter() - t0))
        med = {c: float(np.median(r)) for c, r in rates.items()}
        for c, r in rates.items():
            print("%-8s N = %d, %d SQP, %s payload rows: %.0f traj/s  [%.0f, %.0f] over %d alternating repeats"
                  % (name, N, sqp, c, med[c], min(r), max(r), args.repeats))
        for c in ("zeros", "mixed"):
            print("%-8s time of the %s table against none: %+.2f %% (median against median)" % (name, c, 100.0 * (med["none"] / med[c] - 1.0)))


if __name__ == "__main__":
    main()
