#!/usr/bin/env python3
"""Limits of retimed plans: device time of mpcmp_limits_retimed_batch_device beside mpcmp_limits_batch_device in the same process, at the same B and
n_pts, for one arm and for two; the route call at M = 3; mpcmp_profile_scale_batch_device; and how often a retimed plan leaves its limits between
the grid points.

No solve: the plans are the jerk-limited rest-to-rest moves of the benchmark scenarios (Solver.warm_start_jerk; num_seg 4, for two arms 6), checked under the
configuration's tables with the reference benchmark's tool speed limits 1.7 m/s and 2.5 rad/s, tol 1e-6.  A two-arm plan runs two such moves on
the first one's clock (the second arm's velocities and accelerations rescaled to it).  A route is four moves in a row through three random via
configurations, at rest at each (B routes = 4 B leg slots).  The profiles come from mpcmp_retime_batch_device / mpcmp_retime_route_batch_device at
n_grid.  Device events around the *_device calls on a torch stream, --rounds rounds after one warm-up round, medians reported.
Prints one JSON line.  usage: retimed_check_bench.py [--B 1024] [--n-pts 200] [--n-grid 200] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
NAMES = ("Q", "QD", "QDD", "TAU", "HEIGHT", "TOOL_LIN", "TOOL_ANG")


def rest(x):
    x = np.array(x); x[:, 7:] = 0.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n-pts", type=int, default=200)
    ap.add_argument("--n-grid", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    import mpc_motion_planner_amd as M
    from mpc_motion_planner_amd import scenarios
    B, n_pts, n_grid, nseg, nvia = a.B, a.n_pts, a.n_grid, 4, 3
    L = B * (nvia + 1)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    cfg = M.default_config(nseg, 1, margins=MARGINS)
    one = M.Solver(cfg, L)
    # one arm: B moves; routes: L moves through the points P_0 .. P_4 of every route
    x0, xf = scenarios.make_batch(B, MARGINS)
    sx1, su1, sT1 = one.warm_start_jerk(rest(x0), rest(xf), jmax)
    pts = [rest(scenarios.make_batch(B, MARGINS, stream_offset=(3 + m) * B)[0]) for m in range(nvia + 2)]
    l0 = np.stack(pts[:-1], axis=1).reshape(L, 14); lf = np.stack(pts[1:], axis=1).reshape(L, 14)
    rx, ru, rT = one.warm_start_jerk(l0, lf, jmax)
    # two arms (num_seg 6: a two-arm context takes 6 or 8): the second arm runs another move on the first one's clock
    cfg2 = M.default_config(6, 1, margins=MARGINS)
    gen = M.Solver(cfg2, B)
    ax, au, aT = gen.warm_start_jerk(rest(x0), rest(xf), jmax)
    ox, ou, oT = gen.warm_start_jerk(rest(scenarios.make_batch(B, MARGINS, stream_offset=B)[0]), rest(scenarios.make_batch(B, MARGINS, stream_offset=2 * B)[1]), jmax)
    k = (oT / aT)[:, None, None]
    sx2 = np.concatenate([ax[:, :, :7], ox[:, :, :7], ax[:, :, 7:], ox[:, :, 7:] * k], axis=2)
    su2 = np.concatenate([au, ou * k * k], axis=2)
    two = M.Solver(cfg2, B, models=M.arm_models(M.DUAL_BASES))
    spec, rspec = M.limits_spec(1e-6, 1.7, 2.5), M.retime_spec(1.7, 2.5)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1)

    def dev(x):
        with torch.cuda.stream(stream):
            return torch.from_numpy(np.ascontiguousarray(x)).cuda()

    def records(n):
        with torch.cuda.stream(stream):
            return torch.zeros(n * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    res = {"B": B, "n_pts": n_pts, "n_grid": n_grid, "rounds": a.rounds, "ms_median": {}, "ms_all": {}}
    stats = {}
    for tag, s, hx, hu, hT, route in (("one_arm", one, sx1, su1, sT1, False), ("two_arms", two, sx2, su2, aT, False), ("routes_M3", one, rx, ru, rT, True)):
        n = hT.shape[0]
        dx, du, dT = dev(hx), dev(hu), dev(hT)
        dprof, dfac = dev(np.zeros((n, n_grid + 1, 2))), dev(np.full(n, 1.0))
        drt = dev(np.zeros(n * max(M.RETIME_DTYPE.itemsize, M.ROUTE_RETIME_DTYPE.itemsize) // 8))
        dlim, dret, dTn = records(n), records(n), dev(np.zeros(n))
        p = [t.data_ptr() for t in (dx, du, dT)]
        if route:
            calls = {"retime_route": lambda: s.retime_route_device(B, nvia, *p, n_grid, dprof.data_ptr(), drt.data_ptr(), 0, rspec, stream=st),
                     "limits_legs": lambda: s.limits_device(n, *p, n_pts, dlim.data_ptr(), spec, stream=st),
                     "limits_retimed_route": lambda: s.limits_retimed_route_device(B, nvia, *p, n_grid, dprof.data_ptr(), n_pts, dret.data_ptr(),
                                                                                   dTn.data_ptr(), spec, stream=st)}
        else:
            calls = {"retime": lambda: s.retime_device(n, *p, n_grid, dprof.data_ptr(), drt.data_ptr(), rspec, stream=st),
                     "limits": lambda: s.limits_device(n, *p, n_pts, dlim.data_ptr(), spec, stream=st),
                     "limits_retimed": lambda: s.limits_retimed_device(n, *p, n_grid, dprof.data_ptr(), n_pts, dret.data_ptr(), dTn.data_ptr(), spec, stream=st)}
        ms = {k: [] for k in calls}
        for rnd in range(a.rounds + 1):
            for k, fn in calls.items():
                t = timed(fn)
                if rnd:
                    ms[k].append(t)
        ms["profile_scale"] = [timed(lambda: s.profile_scale_device(n, n_grid, dfac.data_ptr(), dprof.data_ptr(), stream=st)) for _ in range(a.rounds + 1)][1:]
        res["ms_median"][tag] = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        res["ms_all"][tag] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
        nrec = B if route else n
        lim = np.frombuffer(dret.cpu().numpy().tobytes(), dtype=M.LIMITS_DTYPE)[:nrec]
        ok = (lim["status"] & M.LIM_NAN) == 0
        G = lim[ok]
        stats[tag] = {"checked": int(ok.sum()), "failed_profiles": int((~ok).sum()),
                      "share_over": {NAMES[g]: round(float(((G["status"] >> g) & 1).mean()), 4) for g in range(7)} if G.size else {},
                      "excess_max": {NAMES[g]: float(G["excess"][:, g].max()) for g in (2, 3)} if G.size else {},
                      "stretch_median": float(np.median(G["stretch"])) if G.size else None, "stretch_max": float(G["stretch"].max()) if G.size else None}
    m = res["ms_median"]
    res["ratio_to_limits"] = {"one_arm": round(m["one_arm"]["limits_retimed"] / m["one_arm"]["limits"], 3),
                              "two_arms": round(m["two_arms"]["limits_retimed"] / m["two_arms"]["limits"], 3)}
    # per sample: the route call takes n_pts + 1 samples per ROUTE, the per-leg limits call beside it n_pts + 1 per LEG
    res["ns_per_sample"] = {"one_arm": {k: round(1e6 * m["one_arm"][k] / (B * (n_pts + 1)), 3) for k in ("limits", "limits_retimed")},
                            "two_arms": {k: round(1e6 * m["two_arms"][k] / (B * (n_pts + 1)), 3) for k in ("limits", "limits_retimed")},
                            "routes_M3": {"limits_legs": round(1e6 * m["routes_M3"]["limits_legs"] / (L * (n_pts + 1)), 3),
                                          "limits_retimed_route": round(1e6 * m["routes_M3"]["limits_retimed_route"] / (B * (n_pts + 1)), 3)}}
    res["retimed"] = stats
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
