#!/usr/bin/env python3
"""Route retiming: device time of mpcmp_retime_route_batch_device beside mpcmp_retime_batch_device on the same L = B (M + 1) legs, and what one
profile across the via points gains over retiming leg by leg, on solved routes.

B rest-to-rest routes (the benchmark's postures with the end velocities set to 0: a moving end of a route is pinned to x == 1 and would fail
under a reduced-speed row before anything is retimed) with M in {1, 3} vias (the midpoints of start and target plus a seeded offset, chord rule at
--speed) are solved once per M at N = 13, 20 SQP iterations, from the jerk-limited start.  They are then retimed under a reduced-speed row (velocity
margin 0.7 instead of the 0.9 they were solved with) and the reference benchmark's tool limits 1.7 m/s and 2.5 rad/s, as routes and leg by leg.
With --speed 1 the vias are passed at up to 0.9 of the velocity limit, which the row does not allow: leg by leg such a route is infeasible.
A route that fails does so early in its backward pass, so the two times compare like with like only where the feasible shares are alike.  Both calls do the same work per grid point
(the record of a point, the pair elimination, the forward step); the route kernel does it with B waves instead of L.  The per-leg call is the
yardstick.  Device events around the *_device calls on a torch stream, --rounds rounds, medians reported; the first round is a warm-up and is dropped.
Reported per M: the two times and their ratio, the share of routes whose legs are all feasible leg by leg and the share feasible as routes, and
the median T_new of both over the routes feasible both ways (leg by leg: the sum of the legs' T_new).
Prints one JSON line.  usage: route_retime_bench.py [--B 1024] [--n-grid 200] [--rounds 5] [--speed 1.0]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
SLOW = (0.9, 0.7, 0.5, 0.9, 0.1)


def vias(M, x0, xf, nvia, seed=3, spread=0.25):
    cfg = M.default_config(2, 1, margins=MARGINS)
    lo, hi = np.array(cfg.lbx[:7]), np.array(cfg.ubx[:7])
    r = np.random.default_rng(seed)
    f = (np.arange(nvia) + 1.0) / (nvia + 1.0)
    via = x0[:, None, :7] + f[None, :, None] * (xf[:, None, :7] - x0[:, None, :7]) + r.uniform(-spread, spread, (x0.shape[0], nvia, 7))
    return np.ascontiguousarray(np.clip(via, lo + 0.05, hi - 0.05))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-grid", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--speed", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, n, nseg = a.B, a.n_grid, 4
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    spec = M.retime_spec(1.7, 2.5)
    x0, xf = scenarios.make_batch(B, MARGINS)
    x0[:, 7:] = 0.0; xf[:, 7:] = 0.0
    stream = torch.cuda.Stream()
    st = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    res = {"B": B, "n_grid": n, "rounds": a.rounds, "N": 3 * nseg + 1, "speed": a.speed}
    for nvia in (1, 3):
        L = B * (nvia + 1)
        s = M.Solver(M.default_config(nseg, 20, margins=MARGINS), L)
        r = s.solve_route(x0, vias(M, x0, xf, nvia), xf, speed=a.speed, jmax=jmax)
        ok = (r["route_info"]["status"] & (M.STATUS_HARD | M.STATUS_OUTSIDE_TOL | M.STATUS_T_OUT_OF_BOX)) == 0
        s.set_bounds(np.repeat(M.bounds_from_margins(*SLOW), L))
        with torch.cuda.stream(stream):
            d = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
            sx, su, sT = [torch.from_numpy(r[k]).cuda() for k in ("sol_x", "sol_u", "sol_T")]
            prof_r, prof_l, leg_T = d(L, n + 1, 2), d(L, n + 1, 2), d(L)
            rec_r = torch.zeros(B * M.ROUTE_RETIME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            rec_l = torch.zeros(L * M.RETIME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        traj = (sx.data_ptr(), su.data_ptr(), sT.data_ptr())
        ms = {"route": [], "legs": []}
        for rnd in range(a.rounds + 1):
            t = {"route": timed(lambda: s.retime_route_device(B, nvia, *traj, n, prof_r.data_ptr(), rec_r.data_ptr(), leg_T.data_ptr(), spec, stream=st)),
                 "legs": timed(lambda: s.retime_device(L, *traj, n, prof_l.data_ptr(), rec_l.data_ptr(), spec, stream=st))}
            if rnd:
                for k, v in t.items():
                    ms[k].append(v)
        route = np.frombuffer(rec_r.cpu().numpy().tobytes(), dtype=M.ROUTE_RETIME_DTYPE)
        legs = np.frombuffer(rec_l.cpu().numpy().tobytes(), dtype=M.RETIME_DTYPE).reshape(B, nvia + 1)
        by_leg, as_route = ok & (legs["status"] == 0).all(axis=1), ok & (route["status"] == 0)
        both = by_leg & as_route
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res["M%d" % nvia] = {"L": L, "routes_clean": int(ok.sum()), "ms_median": {k: round(v, 4) for k, v in med.items()},
                             "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "route_over_legs": round(med["route"] / med["legs"], 3),
                             "share_feasible_leg_by_leg": round(float(by_leg[ok].mean()), 4) if ok.any() else None,
                             "share_feasible_as_routes": round(float(as_route[ok].mean()), 4) if ok.any() else None,
                             "share_of_legs_feasible": round(float((legs["status"] == 0)[ok].mean()), 4) if ok.any() else None,
                             "routes_feasible_both_ways": int(both.sum()),
                             "T_new_median_as_routes": float(np.median(route["T_new"][both])) if both.any() else None,
                             "T_new_median_leg_by_leg": float(np.median(legs["T_new"][both].sum(axis=1))) if both.any() else None,
                             "T_median_as_planned": float(np.median(r["route_T"][both])) if both.any() else None}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
