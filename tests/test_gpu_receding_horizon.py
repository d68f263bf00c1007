"""GPU parity of the receding-horizon driver (mpcmp_rh_run, BASELINE.json configs[4]) at the sizes the N = 13 tests of test_gpu_parity.py do not
reach: N = 19 (k_init<6> -> k_qp3f<6, 1, 5> + k_qp5 -> k_step<6>; two arms: k_init_m / k_qp3<6, 2> / k_step_m) and N = 25 (k_init_m ->
k_qp3f<8, *> + k_qp3<8, *> -> k_step_m), one arm and two, with the dual-arm start guess (k_split_states -> k_warm_jerk -> k_warm_merge) and
k_advance at nx = 28.  Every comparison is against the oracle's restatement of the driver (oracle_py.rh_chain), eager and with graph replay:
states <= 1e-6, |dT| <= 1e-6 T, equal ADMM iteration counts, status words, ARRIVED bits and re-solve counts.  Run with -m gpu."""
import time

import numpy as np
import pytest

import oracle_py as o

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
CASES = [(6, 1), (8, 1), (6, 2), (8, 2)]          # (num_seg, arms): N = 19 and N = 25, single and dual arm
IDS = ["n19", "n25", "dual_n19", "dual_n25"]


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def dual_states(B, off=0):
    from mpc_motion_planner_amd import scenarios
    a0, af = scenarios.make_batch(B, MARGINS, stream_offset=off)
    b0, bf = scenarios.make_batch(B, MARGINS, stream_offset=off + 7919)
    x0 = np.stack([o.merge_arm_states([a0[b], b0[b]]) for b in range(B)])
    xf = np.stack([o.merge_arm_states([af[b], bf[b]]) for b in range(B)])
    return x0, xf


def _solver(M, cfg, narm, B):
    return M.Solver(cfg, B, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)


def _omodels(narm):
    return o.arm_models(o.DUAL_BASES) if narm == 2 else None


def _configs(M, nseg, flags_on=True, **kw):
    """the device configuration (flags 0: the driver's defaults, carried multipliers and warm QP duals; -1: both off) and the oracle's with the
    same meaning spelled out"""
    f = 1 if flags_on else 0
    dev = M.default_config(nseg, 2, margins=MARGINS, **kw) if flags_on else \
        M.default_config(nseg, 2, margins=MARGINS, qp_warm_start=-1, carry_multipliers=-1, **kw)
    return dev, o.default_config(nseg, 2, margins=MARGINS, carry_multipliers=f, qp_warm_start=f, **kw)


def _check_step(M, s, ch, k, ctx, stats=True):
    """the device after step k + 1 against the oracle chain's record of that step"""
    xg, sx, su, sT, info = s.rh_get()
    ret, Tr = ch["hist_retired"][k], ch["hist_T"][k]
    assert np.abs(xg - ch["hist_x"][k]).max() <= 1e-6, (ctx, k, np.abs(xg - ch["hist_x"][k]).max())
    assert np.all(np.abs(sT - Tr) <= 1e-6 * Tr), (ctx, k, sT, Tr)
    assert np.array_equal(info["qp_iters_total"], ch["hist_its"][k]), (ctx, k, info["qp_iters_total"], ch["hist_its"][k])
    assert np.array_equal(info["status"] & 63, ch["hist_status"][k]), (ctx, k, info["status"], ch["hist_status"][k])
    assert np.array_equal((info["status"] & M.STATUS_ARRIVED) != 0, ret), (ctx, k, info["status"], ret)
    if stats:
        assert s.rh_stats() == (ch["hist_n_solves"][k], int(ret.sum())), (ctx, k, s.rh_stats(), ch["hist_n_solves"][k], int(ret.sum()))
    return xg, sx, su, sT, info


# ---- (a) parity across sizes and start flags -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", CASES, ids=IDS)
@pytest.mark.parametrize("flags_on", [True, False], ids=["driver_defaults", "flags_off"])
def test_receding_horizon_vs_oracle_n19_n25(M, nseg, narm, flags_on):
    """4 steps of 0.05 s on 5 (one arm) or 4 (two arms) instances, eager and graph replay, against the oracle chain; graph replay of 2 + 2 steps equals
    4 steps bit for bit"""
    from mpc_motion_planner_amd import scenarios
    cfg, ocfg = _configs(M, nseg, flags_on)
    x0, xf = scenarios.make_batch(5, MARGINS, stream_offset=40) if narm == 1 else dual_states(4, off=50)
    B, steps, dt = len(x0), 4, 0.05
    ch = o.rh_chain(ocfg, x0, xf, steps, dt, models=_omodels(narm))
    outs = {}
    for use_graph in (False, True):
        s = _solver(M, cfg, narm, B)
        s.rh_init(x0, xf)
        s.rh_run(steps, dt, use_graph=use_graph)
        outs[use_graph] = _check_step(M, s, ch, steps - 1, (nseg, narm, flags_on, use_graph))
        assert np.all((outs[use_graph][4]["status"] & 7) == 0)
    s = _solver(M, cfg, narm, B)
    s.rh_init(x0, xf)
    s.rh_run(2, dt, use_graph=True); s.rh_run(2, dt, use_graph=True)
    out = s.rh_get()
    for a, b in zip(out, outs[True]):
        assert np.array_equal(a, b)
    assert s.rh_stats() == (ch["n_solves"], int(ch["retired"].sum()))


# ---- (b) arrival, one step at a time ---------------------------------------------------------------------------------------------------
ALL_RETIRED_WALL_S = 0.5


def _arrival_setup(M, nseg, narm):
    """control periods of 0.4 s: the instances retire at different steps (one arm: steps 3 - 8 of 6 instances; two arms: steps 5, 7, 7, 8)"""
    from mpc_motion_planner_amd import scenarios
    cfg, ocfg = _configs(M, nseg, True)
    x0, xf = scenarios.make_batch(6, stream_offset=900) if narm == 1 else dual_states(4, off=50)
    return cfg, ocfg, x0, xf, 0.4


@pytest.mark.parametrize("nseg,narm", CASES, ids=IDS)
def test_receding_horizon_arrival_stepwise_vs_oracle(M, nseg, narm):
    """rh_run(1) repeated, compared with the oracle chain after every step: each ARRIVED bit appears at the oracle's step; from its arrival on, a retired
    instance's state, solution, final time and record stay bitwise frozen while the others go on; once all have arrived, 3 more steps change nothing
    and solve nothing.  At N = 25 a retired instance's QP kernels still run (no early exit in k_qp3f / k_qp3<8, *>); for two arms their exchange
    slots must not hold the pair up: the 3 all-retired steps of the captured graph take well under ALL_RETIRED_WALL_S (a few ms are expected; the
    bound only catches an arm workgroup that polls to the exchange time-out, xch_poll's 2^21 polls, whose length in seconds has not been measured)"""
    cfg, ocfg, x0, xf, dt = _arrival_setup(M, nseg, narm)
    B = len(x0)
    ch = o.rh_chain(ocfg, x0, xf, 12, dt, models=_omodels(narm))
    last = int(ch["retired_at"].max())
    assert ch["retired"].all() and len(set(ch["retired_at"].tolist())) >= 3, ch["retired_at"]      # different steps
    for use_graph in (False, True):
        s = _solver(M, cfg, narm, B)
        s.rh_init(x0, xf)
        frozen = {}
        for k in range(last):
            s.rh_run(1, dt, use_graph=use_graph)
            xg, sx, su, sT, info = _check_step(M, s, ch, k, (nseg, narm, use_graph))
            for b in range(B):
                if ch["retired_at"][b] == k + 1:
                    frozen[b] = (xg[b].copy(), sx[b].copy(), su[b].copy(), sT[b], info[b].copy())
                elif b in frozen:
                    f = frozen[b]
                    assert np.array_equal(xg[b], f[0]) and np.array_equal(sx[b], f[1]) and np.array_equal(su[b], f[2]) and sT[b] == f[3], (b, k)
                    assert info[b].tobytes() == f[4].tobytes(), (b, k, info[b], f[4])
        assert len(frozen) == B
        stats = s.rh_stats()
        assert stats == (ch["n_solves"], B)
        t0 = time.perf_counter()
        s.rh_run(3, dt, use_graph=use_graph)          # (graph: captured in the loop above, same dt)
        wall = time.perf_counter() - t0
        xg, sx, su, sT, info = s.rh_get()
        for b in range(B):
            f = frozen[b]
            assert np.array_equal(xg[b], f[0]) and np.array_equal(sx[b], f[1]) and np.array_equal(su[b], f[2]) and sT[b] == f[3], b
            assert info[b].tobytes() == f[4].tobytes(), (b, info[b], f[4])
        assert s.rh_stats() == stats
        print("all-retired steps, N = %d, %d arm(s), %s: 3 steps in %.2f ms" % (3 * nseg + 1, narm, "graph" if use_graph else "eager", 1e3 * wall))
        if use_graph:
            assert wall < ALL_RETIRED_WALL_S, wall


# ---- (c) restart after a failed solve --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm,ubT", [(6, 1, 1.5), (8, 1, 1.5), (8, 2, 2.0)], ids=["n19", "n25", "dual_n25"])
def test_failed_solve_holds_state_and_restarts_vs_oracle_n19_n25(M, nseg, narm, ubT):
    """a final-time box [0, ubT] too narrow for some instances, not all (the oracle chain says so): their solves end with MPCMP_STATUS_T_OUT_OF_BOX,
    they hold their state and restart from the driver's start guess with zero multipliers (k_init's / k_init_m's alt_x path; two arms: the
    per-arm generator's restart mask over B x 2 arm problems).  [0, 1.5] fails every dual-arm instance of dual_states(4, off=50), so two arms take
    [0, 2.0].  Compared after 1, 2 and 4 steps, eager and (4 steps) graph replay"""
    from mpc_motion_planner_amd import scenarios
    cfg, ocfg = _configs(M, nseg, True, lbT=0.0, ubT=ubT)
    x0, xf = scenarios.make_batch(6, stream_offset=900) if narm == 1 else dual_states(4, off=50)
    B, dt = len(x0), 0.05
    ch = o.rh_chain(ocfg, x0, xf, 4, dt, models=_omodels(narm))
    bad = (ch["hist_status"][0] & 32) != 0
    assert bad.any() and not bad.all(), ch["hist_status"][0]
    assert ch["restarts"].any(), ch["restarts"]
    for steps, use_graph in ((1, False), (2, False), (4, False), (4, True)):
        s = _solver(M, cfg, narm, B)
        s.rh_init(x0, xf)
        s.rh_run(steps, dt, use_graph=use_graph)
        xg = _check_step(M, s, ch, steps - 1, (nseg, narm, steps, use_graph))[0]
        if steps == 1:
            assert np.array_equal(xg[bad], x0[bad])            # held: there is no trajectory to follow


# ---- (d) the two-stream shape ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm,B", [(6, 1, 512), (8, 2, 256)], ids=["n19_B512", "dual_n25_B256"])
def test_receding_horizon_two_streams_vs_oracle(M, nseg, narm, B):
    """batches large enough to be solved as two halves on two streams (dual N = 25: 256 instances = 512 arm workgroups, solve_impl_m's split):
    6 steps, graph replay equal to eager bit for bit; the first instance of each half and the last one follow the oracle chain"""
    from mpc_motion_planner_amd import scenarios
    cfg, ocfg = _configs(M, nseg, True)
    x0, xf = scenarios.make_batch(B, MARGINS, stream_offset=300) if narm == 1 else dual_states(B, off=300)
    steps, dt = 6, 0.02
    idx = [0, (B + 1) // 2, B - 1]
    ch = o.rh_chain(ocfg, x0[idx], xf[idx], steps, dt, models=_omodels(narm))
    outs = {}
    for use_graph in (False, True):
        s = _solver(M, cfg, narm, B)
        s.rh_init(x0, xf)
        s.rh_run(steps, dt, use_graph=use_graph)
        outs[use_graph] = (s.rh_get(), s.rh_stats())
    for a, b in zip(outs[False][0], outs[True][0]):
        assert np.array_equal(a, b)
    assert outs[False][1] == outs[True][1]
    xg, sx, su, sT, info = outs[True][0]
    Tr = ch["T"]
    assert np.abs(xg[idx] - ch["x"]).max() <= 1e-6, np.abs(xg[idx] - ch["x"]).max()
    assert np.all(np.abs(sT[idx] - Tr) <= 1e-6 * Tr), (sT[idx], Tr)
    assert np.array_equal(info["qp_iters_total"][idx], ch["its"]), (info["qp_iters_total"][idx], ch["its"])
    assert np.array_equal(info["status"][idx] & 63, ch["status"]) and np.array_equal((info["status"][idx] & M.STATUS_ARRIVED) != 0, ch["retired"])
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(sT))


# ---- (e) carried multipliers at N = 25 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm", [1, 2], ids=["n25", "dual_n25"])
def test_carried_multipliers_vs_oracle_n25(M, narm):
    """mpcmp_config.carry_multipliers + qp_warm_start on plain N = 25 solves (k_init_m / k_qp3<8, *> / k_step_m: the multiplier block of every
    arm at its own offset): a solve and its re-solve from the solution with the end states re-pinned (motionPlanner.cpp:199-207), the second
    one starting from the multipliers of the first: identical ADMM iteration counts and status words against orc_solve_carry(_multi); after
    mpcmp_reset_multipliers the first solve again, bit for bit"""
    from mpc_motion_planner_amd import scenarios
    nseg, sqp, B = 8, 2, 2
    cfg = M.default_config(nseg, sqp, margins=MARGINS, qp_warm_start=1, carry_multipliers=1)
    ocfg = o.default_config(nseg, sqp, margins=MARGINS, qp_warm_start=1, carry_multipliers=1)
    s = _solver(M, cfg, narm, B)
    if narm == 1:
        x0, xf = scenarios.make_batch(B, MARGINS, stream_offset=900)
        wx, wu, wT = s.warm_start(x0, xf)
    else:
        x0, xf = dual_states(B, off=77)
        N = 3 * nseg + 1
        wx = np.zeros((B, N, 28)); wu = np.zeros((B, N, 14)); wT = np.zeros(B)
        lim = o.default_limits()
        for b in range(B):
            wx[b], wu[b], wT[b] = o.warm_start_jerk_multi(nseg, MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"], x0[b], xf[b])
    sx1, su1, sT1, i1 = s.solve(x0, xf, (wx, wu, wT))
    gx = sx1.copy(); gx[:, 0] = x0; gx[:, -1] = xf
    sx2, su2, sT2, i2 = s.solve(x0, xf, (gx, su1, sT1))
    s.reset_multipliers()
    sx3, su3, sT3, i3 = s.solve(x0, xf, (wx, wu, wT))
    assert np.array_equal(sx3, sx1) and np.array_equal(sT3, sT1) and np.array_equal(i3["qp_iters_total"], i1["qp_iters_total"])
    models = _omodels(narm)
    for b in range(B):
        if narm == 1:
            xs, us, T, oi, lam = o.solve_carry(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        else:
            xs, us, T, oi, lam = o.solve_carry_multi(models, ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert oi.qp_iters_total == i1["qp_iters_total"][b] and oi.status == i1["status"][b] and abs(sT1[b] - T) <= 1e-6 * T
        g = xs.copy(); g[0] = x0[b]; g[-1] = xf[b]
        if narm == 1:
            xs2, us2, T2, oi2, _ = o.solve_carry(ocfg, x0[b], xf[b], g, us, T, lam=lam)
        else:
            xs2, us2, T2, oi2, _ = o.solve_carry_multi(models, ocfg, x0[b], xf[b], g, us, T, lam=lam)
        assert oi2.qp_iters_total == i2["qp_iters_total"][b] and oi2.status == i2["status"][b], (b, oi2.qp_iters_total, i2["qp_iters_total"][b])
        assert abs(sT2[b] - T2) <= 1e-6 * T2 and np.abs(sx2[b] - xs2).max() <= 1e-5
        assert oi2.qp_iters_total != oi.qp_iters_total or not np.array_equal(xs2, xs)      # (the re-solve is another solve)
