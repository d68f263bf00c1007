#!/usr/bin/env python3
"""Via-point routes: device time of mpcmp_solve_route_batch_device beside the plain solve of as many problems as it has legs.

B = 256 routes with M = 3 vias (L = 1,024 legs) at N = 13, 20 SQP iterations, jerk-limited start guess; next to it mpcmp_solve_batch_device of 1,024
problems from the same scenario stream.  Vias: the points that divide the straight joint-space line into M + 1 parts, plus a seeded offset.
Device events on a torch stream, --rounds alternating rounds, medians reported; the first round is a warm-up and is dropped.
The three new kernels (k_route_legs, k_route_join, k_sample_route) are timed by events around their own *_device entry points, one launch each;
mpcmp_kernel_timing reports the dominant QP kernel only, and its figure for the route solve and the plain solve is printed beside them.
Then the sweep: speed = 0.25, 0.5, 0.75, 1 -> the share of routes with status 0, the share whose status has no inadmissible bit, the mean route_T of
those, and the mean acceleration jump at the vias.
Prints one JSON line.  usage: route_bench.py [--B 256] [--M 3] [--rounds 4] [--n-pts 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
BAD = 1 | 2 | 4 | 16 | 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--M", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--n-pts", type=int, default=200)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, nvia, n_pts = a.B, a.M, a.n_pts
    L = B * (nvia + 1)
    cfg = M.default_config(4, 20, margins=MARGINS)
    s = M.Solver(cfg, L)
    N = s.N
    x0, xf = scenarios.make_batch(B, MARGINS)
    p0, pf = scenarios.make_batch(L, MARGINS)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    f = (np.arange(nvia) + 1.0) / (nvia + 1.0)
    lo, hi = np.array(cfg.lbx[:7]) + 0.05, np.array(cfg.ubx[:7]) - 0.05
    via = x0[:, None, :7] + f[None, :, None] * (xf[:, None, :7] - x0[:, None, :7]) + np.random.default_rng(1).uniform(-0.25, 0.25, (B, nvia, 7))
    via = np.ascontiguousarray(np.clip(via, lo, hi))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
        rec = lambda n, dt: torch.zeros(n * dt.itemsize, dtype=torch.uint8, device="cuda")      # noqa: E731
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
        tx0, txf, tvia, tp0, tpf, tsp = up(x0), up(xf), up(via), up(p0), up(pf), d(B)
        wx, wu, wT, sx, su, sT = d(L, N, 14), d(L, N, 7), d(L), d(L, N, 14), d(L, N, 7), d(L)
        l0, lf, rT, vo, smp = d(L, 14), d(L, 14), d(B), d(B, max(nvia, 1), 7), d(B, n_pts + 1, 29)
        tinfo, rinfo, seam = rec(L, M.INFO_DTYPE), rec(B, M.INFO_DTYPE), rec(B, M.ROUTE_SEAM_DTYPE)
    stream.synchronize()
    st = stream.cuda_stream
    P = lambda t: t.data_ptr()      # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    def route(speed):
        tsp.fill_(speed)
        s.solve_route_device(B, nvia, P(tx0), P(tvia), P(txf), P(sx), P(su), P(sT), P(rT), P(rinfo), P(seam), info=P(tinfo), speed=P(tsp), jmax=jmax,
                             via_qd_out=P(vo), stream=st)

    def plain():
        s.warm_start_jerk_device(L, P(tp0), P(tpf), jmax, P(wx), P(wu), P(wT), stream=st)
        s.solve_device(L, P(tp0), P(tpf), P(sx), P(su), P(sT), P(tinfo), warm=(P(wx), P(wu), P(wT)), stream=st)

    s.kernel_timing(reset=True)
    ms = {k: [] for k in ("route_solve", "plain_solve", "k_route_legs", "k_route_join", "k_sample_route")}
    qp = {"route_solve": [], "plain_solve": []}
    for rnd in range(a.rounds + 1):
        t = {}
        for name, fn in (("plain_solve", plain), ("route_solve", lambda: route(0.5))):
            with torch.cuda.stream(stream):
                t[name] = timed(fn)
            qp_ms = s.kernel_timing(reset=True)[1]
            if rnd:
                qp[name].append(qp_ms)
        with torch.cuda.stream(stream):                      # (the route solve is the last one: sx / su / sT hold its legs)
            t["k_route_legs"] = timed(lambda: s.route_legs_device(B, nvia, P(tx0), P(tvia), P(txf), P(l0), P(lf), speed=P(tsp), via_qd_out=P(vo), stream=st))
            t["k_route_join"] = timed(lambda: s.route_join_device(B, nvia, P(sx), P(su), P(sT), P(tinfo), P(rT), P(rinfo), P(seam), stream=st))
            t["k_sample_route"] = timed(lambda: s.sample_route_device(B, nvia, P(sx), P(su), P(sT), n_pts, P(smp), stream=st))
        if rnd:
            for k, v in t.items():
                ms[k].append(v)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    sweep = {}
    for speed in (0.25, 0.5, 0.75, 1.0):
        with torch.cuda.stream(stream):
            route(speed)
        stream.synchronize()
        ri = rinfo.cpu().numpy().view(M.INFO_DTYPE); sm = seam.cpu().numpy().view(M.ROUTE_SEAM_DTYPE); T = rT.cpu().numpy()
        ok = (ri["status"] & BAD) == 0
        sweep[str(speed)] = {"share_status_0": round(float((ri["status"] == 0).mean()), 4), "share_admissible": round(float(ok.mean()), 4),
                             "mean_route_T_admissible": round(float(T[ok].mean()), 4) if ok.any() else None,
                             "mean_route_T_all_finite": round(float(T[np.isfinite(T)].mean()), 4),
                             "mean_acc_jump": round(float(sm["acc_jump_inf"][ok].mean()), 3) if ok.any() else None,
                             "mean_qp_iters_per_leg": round(float(ri["qp_iters_total"].mean()) / (nvia + 1), 1)}
    res = {"B": B, "M": nvia, "legs": L, "N": N, "n_pts": n_pts, "rounds": a.rounds,
           "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "qp_kernel_ms_median": {k: round(float(np.median(v)), 4) for k, v in qp.items()},
           "routes_per_s": round(B / (med["route_solve"] * 1e-3)), "legs_per_s": round(L / (med["route_solve"] * 1e-3)),
           "plain_problems_per_s": round(L / (med["plain_solve"] * 1e-3)),
           "route_over_plain": round(med["route_solve"] / med["plain_solve"], 4), "speed_sweep": sweep}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
