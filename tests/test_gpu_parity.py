"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on the same inputs. Run with -m gpu."""
import json
import os

import numpy as np
import pytest

import oracle_py as o

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _cfgs(M, nseg, sqp, **kw):
    return M.default_config(nseg, sqp, margins=MARGINS, **kw), o.default_config(nseg, sqp, margins=MARGINS, **kw)


def test_models_identical(M):
    a, b = M.default_model(), o.default_model()
    for f in ["R0", "p", "mass", "com", "I", "tool", "link8", "gravity"]:
        assert np.array_equal(np.array(getattr(a, f)), np.array(getattr(b, f))), f


def test_rnea_vs_oracle_and_golden(M, golden_dir):
    cfg, _ = _cfgs(M, 4, 1)
    s = M.Solver(cfg, 8)
    k = np.loadtxt(os.path.join(golden_dir, "kat_rnea.csv"), delimiter=",")
    tau = s.rnea(k[:, 1:8], k[:, 8:15], k[:, 15:22])
    assert np.abs(tau - k[:, 22:29]).max() < 2.5e-4            # reference's stored Pinocchio outputs (6 s.f. inputs)
    ref = np.stack([o.rnea(r[1:8], r[8:15], r[15:22]) for r in k])
    assert np.abs(tau - ref).max() < 1e-11                     # fp64 tolerance vs oracle (|tau| ~ 60)
    # ragged size: 1 element, and a size that is not a multiple of the workgroup
    rng = np.random.default_rng(0)
    for nn in (1, 67):
        q, v, a = rng.uniform(-2, 2, (nn, 7)), rng.uniform(-2, 2, (nn, 7)), rng.uniform(-10, 10, (nn, 7))
        ref = np.stack([o.rnea(q[i], v[i], a[i]) for i in range(nn)])
        assert np.abs(s.rnea(q, v, a) - ref).max() < 1e-11


def test_eval_constraints_vs_oracle(M):
    cfg, _ = _cfgs(M, 4, 1)
    s = M.Solver(cfg, 8)
    rng = np.random.default_rng(1)
    lim = o.default_limits()
    for nn in (1, 13, 40):                                     # below, equal to and above one node chunk
        x = np.concatenate([rng.uniform(lim["qmin"], lim["qmax"], (nn, 7)), rng.uniform(-1, 1, (nn, 7)) * lim["vmax"]], axis=1)
        u = rng.uniform(-1, 1, (nn, 7)) * lim["amax"]
        g, G = s.eval_constraints(x, u)
        for i in range(nn):
            g0, G0 = o.eval_constraints(x[i], u[i], quirk=1)
            assert np.abs(g[i] - g0).max() < 1e-11
            assert np.abs(G[i] - G0).max() < 1e-10 * (1 + np.abs(G0).max())


def test_builtin_warm_start_vs_oracle(M):
    cfg, ocfg = _cfgs(M, 4, 1)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(16)
    s = M.Solver(cfg, 16)
    wx, wu, wT = s.warm_start(x0, xf)
    for b in range(16):
        xg, ug, Tg = o.warm_start(ocfg, x0[b], xf[b])
        assert abs(wT[b] - Tg) < 1e-12 * Tg
        assert np.abs(wx[b] - xg).max() < 1e-10 and np.abs(wu[b] - ug).max() < 1e-9


def _qp_case(M, nseg, B, qp_iters):
    cfg, ocfg = _cfgs(M, nseg, 1, qp_iters=qp_iters)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(B)
    xs = np.zeros((B, 3 * nseg + 1, 14)); us = np.zeros((B, 3 * nseg + 1, 7)); T = np.zeros(B)
    for b in range(B):
        xs[b], us[b], T[b] = o.warm_start(ocfg, x0[b], xf[b])
    s = M.Solver(cfg, B)
    p, y, it = s.qp(x0, xf, xs, us, T)
    for b in range(B):
        p0, y0, it0 = o.debug_qp(ocfg, x0[b], xf[b], xs[b], us[b], T[b])
        assert it[b] == it0
        sc = 1 + np.abs(p0).max()
        assert np.abs(p[b] - p0).max() < 1e-7 * sc, (b, np.abs(p[b] - p0).max())
        assert np.abs(y[b] - y0).max() < 1e-6 * (1 + np.abs(y0).max()), (b, np.abs(y[b] - y0).max())


def test_qp_few_iterations_vs_oracle(M):
    _qp_case(M, 4, 3, 5)         # exercises assembly + factorisation + the iteration body


def test_qp_full_vs_oracle(M):
    _qp_case(M, 4, 4, 700)       # includes termination tests every 25 iterations


@pytest.mark.parametrize("kern", ["3", "4"])
def test_n13_e_free_kernels_vs_oracle(M, kern, monkeypatch):
    """N = 13 through the E-free kernels (MPCMP_QP13 picks them at mpcmp_create): 3 = k_qp3f + k_qp3<4, 1>; 4 = k_qp3f<4, 1, 4> + k_qp4, the
    384-thread / 80 KB loop sized for two OCPs per CU (it does not co-reside at its 168 VGPRs, kept as a measured
    alternative).  One full QP and a 3-iteration solve against the oracle, identical ADMM iteration counts."""
    monkeypatch.setenv("MPCMP_QP13", kern)
    if kern == "4":     # k_qp4 is an experiment outside the product build (tools/experiments/qp_kernel_v4.hpp, -DMPCMP_WITH_QP4): the library must say so
        try:
            M.Solver(_cfgs(M, 4, 3)[0], 1)
        except M.MpcmpError as e:
            assert "k_qp4" in str(e)
            pytest.skip("library built without k_qp4 (the product build)")
    _qp_case(M, 4, 3, 700)
    cfg, ocfg = _cfgs(M, 4, 3)
    from mpc_motion_planner_amd import scenarios
    B = 3
    x0, xf = scenarios.make_batch(B, stream_offset=40)
    s = M.Solver(cfg, B)
    wx = np.zeros((B, 13, 14)); wu = np.zeros((B, 13, 7)); wT = np.zeros(B)
    for b in range(B):
        wx[b], wu[b], wT[b] = o.warm_start(ocfg, x0[b], xf[b])
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    for b in range(B):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert abs(sT[b] - T) <= 1e-6 * T and np.abs(sx[b] - xs).max() <= 1e-6
        assert info["qp_iters_total"][b] == oi.qp_iters_total and info["status"][b] == oi.status


@pytest.mark.parametrize("nseg,B,iters", [(6, 2, 5), (6, 3, 700), (8, 2, 5), (8, 3, 700)])
def test_qp3_vs_oracle(M, nseg, B, iters):
    """N = 19 as shipped (default kernel: k_qp3f<6, 1, 5> + k_qp5, factor resident on the CU) and N = 25 (k_qp3f + k_qp3): T bordered out —
    one QP against the oracle's skyline Cholesky"""
    _qp_case(M, nseg, B, iters)


def test_n19_both_loop_kernels_vs_oracle(M, monkeypatch):
    """N = 19 through BOTH loop kernels (MPCMP_QP19 picks at mpcmp_create): 5 = k_qp5 (default: G, E, S^-1 blocks in registers, loaded once),
    3 = k_qp3 (E-free, blocks re-read every test period).  One full QP and a 2-iteration solve each against the oracle, identical ADMM
    iteration counts; the two kernels' results agree to round-off."""
    from mpc_motion_planner_amd import scenarios
    res = {}
    for kern in ("5", "3"):
        monkeypatch.setenv("MPCMP_QP19", kern)
        _qp_case(M, 6, 3, 700)
        cfg, ocfg = _cfgs(M, 6, 2)
        B = 3
        x0, xf = scenarios.make_batch(B, stream_offset=70)
        s = M.Solver(cfg, B)
        assert s.kernel_timing()[0] == ("k_qp5" if kern == "5" else "k_qp3")
        wx = np.zeros((B, 19, 14)); wu = np.zeros((B, 19, 7)); wT = np.zeros(B)
        for b in range(B):
            wx[b], wu[b], wT[b] = o.warm_start(ocfg, x0[b], xf[b])
        sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
        for b in range(B):
            xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
            assert abs(sT[b] - T) <= 1e-6 * T and np.abs(sx[b] - xs).max() <= 1e-6
            assert info["qp_iters_total"][b] == oi.qp_iters_total and info["status"][b] == oi.status
        res[kern] = (sx, sT, info["qp_iters_total"].copy())
    assert np.array_equal(res["5"][2], res["3"][2])
    assert np.abs(res["5"][0] - res["3"][0]).max() <= 1e-7 and np.abs(res["5"][1] - res["3"][1]).max() <= 1e-8


@pytest.mark.parametrize("nseg,sqp,B,kern", [(4, 6, 3, ""), (4, 20, 2, ""), (6, 4, 3, ""), (6, 4, 3, "qp19=3"), (8, 4, 2, ""), (2, 4, 2, ""), (1, 4, 2, ""), (4, 4, 2, "qp13=3")])
def test_solve_vs_oracle_qp_warm_start(M, nseg, sqp, B, kern, monkeypatch):
    """mpcmp_config.qp_warm_start = 1 (opt-in: the QPs after the first start from the NLP multipliers, y_0 = lambda_k, x_0 = 0, z_0 = clip(0, l, u))
    through every loop kernel — k_qp2 (N = 7, 13), k_qp5 and k_qp3 (N = 19), k_qp3 (N = 25, and N = 13 on request), the generic k_qp (N = 4) —
    against the oracle with the same flag: identical ADMM iteration counts, step lengths and status words; and the flag does change the run."""
    if kern:
        monkeypatch.setenv("MPCMP_" + kern.split("=")[0].upper(), kern.split("=")[1])
    cfg, ocfg = _cfgs(M, nseg, sqp, qp_warm_start=1)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(B, stream_offset=300)
    N = 3 * nseg + 1
    wx = np.zeros((B, N, 14)); wu = np.zeros((B, N, 7)); wT = np.zeros(B)
    for b in range(B):
        wx[b], wu[b], wT[b] = o.warm_start(ocfg, x0[b], xf[b])
    s = M.Solver(cfg, B)
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    cold = 0
    for b in range(B):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert abs(sT[b] - T) <= 1e-6 * abs(T) and np.abs(sx[b] - xs).max() <= 1e-6 and np.abs(su[b] - us).max() <= 1e-5
        assert info["qp_iters_total"][b] == oi.qp_iters_total and info["last_alpha"][b] == oi.last_alpha and info["status"][b] == oi.status
        cold += o.solve(_cfgs(M, nseg, sqp)[1], x0[b], xf[b], wx[b], wu[b], wT[b])[3].qp_iters_total
    if (nseg, sqp) == (4, 6):       # (the flag changes the run: checked where not every later QP runs into the cap both ways)
        assert cold != int(info["qp_iters_total"].sum())


@pytest.mark.parametrize("nseg,sqp,B", [(4, 2, 4), (4, 20, 3), (6, 2, 3), (6, 20, 2), (8, 2, 3), (8, 20, 2), (2, 3, 2), (1, 3, 2)])
def test_solve_vs_oracle(M, nseg, sqp, B):
    cfg, ocfg = _cfgs(M, nseg, sqp)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(B, stream_offset=100)
    N = 3 * nseg + 1
    wx = np.zeros((B, N, 14)); wu = np.zeros((B, N, 7)); wT = np.zeros(B)
    for b in range(B):
        wx[b], wu[b], wT[b] = o.warm_start(ocfg, x0[b], xf[b])
    s = M.Solver(cfg, B)
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    for b in range(B):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        # tolerance stated by the north star: terminal state and constraint residuals; measured differences are
        # ~1e-9 (different factorisation order: nested-dissection block inverses vs skyline Cholesky)
        assert abs(sT[b] - T) <= 1e-6 * T, (b, sT[b], T)
        assert np.abs(sx[b] - xs).max() <= 1e-6, (b, np.abs(sx[b] - xs).max())
        assert np.abs(su[b] - us).max() <= 1e-5, (b, np.abs(su[b] - us).max())
        assert info["qp_iters_total"][b] == oi.qp_iters_total and info["status"][b] == oi.status and info["qp_capped"][b] == oi.qp_capped
        assert abs(info["viol_l1"][b] - oi.viol_l1) < 1e-6 and abs(info["defect_inf"][b] - oi.defect_inf) < 1e-6
        assert abs(info["term_err_inf"][b] - oi.term_err_inf) < 1e-6 and info["last_alpha"][b] == oi.last_alpha


def test_gold_traj_scenario_on_gpu(M, golden_dir):
    """the one stored solve of the reference (19 nodes, 1 SQP iteration, 700-iteration QP cap) through the HIP path: warm start
    by k_warm_jerk, solve, resample; same fitted tolerances against the stored 201 x 21 MPC samples as the oracle test
    (tests/test_oracle_ocp.py::test_gold_traj_fit), and GPU == oracle on the same guess."""
    from test_oracle_ocp import GOLD_FIT, jerk_warm_start
    g = json.load(open(os.path.join(golden_dir, "gold_traj.json")))
    x0 = np.array(g["q0"] + g["v0"]); xf = np.array(g["qT"] + g["vT"])
    cfg, ocfg = _cfgs(M, 6, 1)
    s = M.Solver(cfg, 1)
    jmax = g["margins"][4] * M.default_limits()["jmax"]
    warm = s.warm_start_jerk(x0[None], xf[None], jmax)
    sx, su, sT, info = s.solve(x0[None], xf[None], warm)
    assert info["qp_iters_total"][0] == 700 and (info["status"][0] & 7) == 0 and info["status"][0] & 8 and info["qp_capped"][0] == 1
    gx = sx.copy(); gx[0, 0] = x0; gx[0, -1] = xf                 # the stored samples were taken after the re-guess (motionPlanner.cpp:199-207)
    smp = s.sample(gx, su, sT, 200)[0]
    assert abs(sT[0] - g["T_mpc"]) < GOLD_FIT["dT"]
    assert np.abs(smp[:, 1:8] - np.array(g["q_mpc"])).max() < GOLD_FIT["dq"]
    assert np.abs(smp[:, 8:15] - np.array(g["v_mpc"])).max() < GOLD_FIT["dv"]
    assert np.abs(smp[:, 15:22] - np.array(g["a_mpc"])).max() < GOLD_FIT["da"]
    xg, ug, Tg = jerk_warm_start(g, x0, xf, 6)
    xs, us, T, oi = o.solve(ocfg, x0, xf, xg, ug, Tg)
    assert abs(sT[0] - T) < 1e-6 and np.abs(sx[0] - xs).max() < 1e-6
    # the solver depth as shipped (2 SQP iterations, motionPlanner.cpp:15)
    cfg2, ocfg2 = _cfgs(M, 6, 2)
    s2 = M.Solver(cfg2, 1)
    sx2, su2, sT2, info2 = s2.solve(x0[None], xf[None], warm)
    xs2, us2, T2, _ = o.solve(ocfg2, x0, xf, xg, ug, Tg)
    assert abs(sT2[0] - T2) < 1e-6 and np.abs(sx2[0] - xs2).max() < 1e-6 and 1.52 < sT2[0] < sT[0]


def test_sample_vs_oracle(M):
    cfg, ocfg = _cfgs(M, 4, 2)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(3, stream_offset=7)
    s = M.Solver(cfg, 3)
    sx, su, sT, _ = s.solve(x0, xf)
    out = s.sample(sx, su, sT, n_pts=200)
    for b in range(3):
        ref = o.sample(4, sx[b], su[b], sT[b], 200)
        assert np.abs(out[b] - ref).max() < 1e-9


def test_builtin_warm_start_solve_and_properties(M):
    """size-independent properties at a larger batch: feasibility of the returned iterate, determinism,
    independence of a problem's result from its position in the batch."""
    cfg, _ = _cfgs(M, 4, 6)
    from mpc_motion_planner_amd import scenarios
    B = 96
    x0, xf = scenarios.make_batch(B)
    s = M.Solver(cfg, B)
    sx, su, sT, info = s.solve(x0, xf)
    assert np.all((info["status"] & 7) == 0) and np.all(np.isfinite(sT))
    sx2, su2, sT2, _ = s.solve(x0, xf)
    assert np.array_equal(sx, sx2) and np.array_equal(sT, sT2)        # bitwise reproducible
    perm = np.random.default_rng(5).permutation(B)
    sx3, _, sT3, _ = s.solve(x0[perm], xf[perm])
    assert np.array_equal(sT3, sT[perm]) and np.array_equal(sx3, sx[perm])
    assert np.median(info["term_err_inf"]) < 2e-2


def test_error_behaviour(M):
    cfg, _ = _cfgs(M, 4, 1)
    s = M.Solver(cfg, 2)
    x0 = np.zeros((3, 14))
    with pytest.raises(M.MpcmpError):
        s.solve(x0, x0)                                    # batch larger than capacity
    bad = M.default_config(3, 1)
    with pytest.raises(M.MpcmpError):
        M.Solver(bad, 1)                                   # unsupported NUM_SEG


def _oracle_rh_chain(ocfg, x0, xf, steps, dt):
    """mpcmp_rh_run restated with the oracle: the shared chain (oracle_py.rh_chain), its final state, final times, iteration counts and status words of
    the last solve executed, retired instances and re-solve count"""
    r = o.rh_chain(ocfg, x0, xf, steps, dt)
    return r["x"], r["T"], r["its"], r["status"], r["retired"], r["n_solves"]


def test_receding_horizon_vs_oracle(M):
    """BASELINE config #5 in miniature: warm-started re-solves + state advance, eager and hipGraph replay; here with both start flags OFF (-1):
    every re-solve starts from lambda = 0 and every QP cold (the round-1..4 behaviour of the driver)"""
    cfg, ocfg = M.default_config(4, 2, margins=MARGINS, qp_warm_start=-1, carry_multipliers=-1), o.default_config(4, 2, margins=MARGINS)
    from mpc_motion_planner_amd import scenarios
    B, steps, dt = 3, 4, 0.05
    x0, xf = scenarios.make_batch(B, stream_offset=40)
    xr, Tr, its, st, ret, ns = _oracle_rh_chain(ocfg, x0, xf, steps, dt)
    for use_graph in (False, True):
        s = M.Solver(cfg, B)
        s.rh_init(x0, xf)
        s.rh_run(steps, dt, use_graph=use_graph)
        xg, sx, su, sT, info = s.rh_get()
        assert np.abs(xg - xr).max() < 1e-6, (use_graph, np.abs(xg - xr).max())
        assert np.abs(sT - Tr).max() < 1e-6 and np.array_equal(info["qp_iters_total"], its)
        assert np.all((info["status"] & 7) == 0) and s.rh_stats() == (ns, 0)
    # graph replay continues where the eager run stopped: run 2 + 2 equals run 4
    s = M.Solver(cfg, B); s.rh_init(x0, xf); s.rh_run(2, dt, use_graph=True); s.rh_run(2, dt, use_graph=True)
    assert np.array_equal(s.rh_get()[0], xg)


@pytest.mark.parametrize("nseg", [4, 6])
def test_carried_multipliers_vs_oracle(M, nseg):
    """(i) the receding-horizon driver's DEFAULT (flags 0 = carry_multipliers + qp_warm_start on inside mpcmp_rh_run): every re-solve starts from the
    multipliers of the one before (k_qp2), eager and graph replay, equal to the flags set to 1 explicitly; (ii) re-solves through the plain solve call on
    one context with the flags set (N = 13: k_qp2, N = 19: k_qp3f + k_qp5), reset in between; against the oracle's chain with the multipliers handed
    from solve to solve: identical ADMM iteration counts"""
    cfg, ocfg = _cfgs(M, nseg, 2, carry_multipliers=1, qp_warm_start=1)
    from mpc_motion_planner_amd import scenarios
    B, steps, dt = 4, 4, 0.02
    x0, xf = scenarios.make_batch(B, stream_offset=900)
    if nseg == 4:
        xc, Tr, its, st, ret, ns = _oracle_rh_chain(ocfg, x0, xf, steps, dt)
        for use_graph in (False, True):
            for c in (M.default_config(nseg, 2, margins=MARGINS), cfg):           # the driver's default, and the flags spelled out
                s = M.Solver(c, B)
                s.rh_init(x0, xf)
                s.rh_run(steps, dt, use_graph=use_graph)
                xg, sx, su, sT, info = s.rh_get()
                assert np.array_equal(info["qp_iters_total"], its), (use_graph, info["qp_iters_total"], its)
                assert np.abs(xg - xc).max() < 1e-6 and np.abs(sT - Tr).max() < 1e-6
                s.rh_init(x0, xf)                                 # (a new set of instances: nothing carried over)
                s.rh_run(steps, dt, use_graph=use_graph)
                assert np.array_equal(s.rh_get()[0], xg)
    # plain solves on one context: solve, re-solve from the solution (motionPlanner.cpp:199-207), reset, solve again
    s = M.Solver(cfg, B)
    wx, wu, wT = s.warm_start(x0, xf)
    sx1, su1, sT1, i1 = s.solve(x0, xf, (wx, wu, wT))
    gx = sx1.copy(); gx[:, 0] = x0; gx[:, -1] = xf
    sx2, su2, sT2, i2 = s.solve(x0, xf, (gx, su1, sT1))
    s.reset_multipliers()
    sx3, su3, sT3, i3 = s.solve(x0, xf, (wx, wu, wT))
    assert np.array_equal(sx3, sx1) and np.array_equal(i3["qp_iters_total"], i1["qp_iters_total"])
    for b in range(B):
        xs, us, T, oi, lam = o.solve_carry(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert oi.qp_iters_total == i1["qp_iters_total"][b] and abs(sT1[b] - T) <= 1e-6 * T
        g = xs.copy(); g[0] = x0[b]; g[-1] = xf[b]
        xs2, us2, T2, oi2, _ = o.solve_carry(ocfg, x0[b], xf[b], g, us, T, lam=lam)
        assert oi2.qp_iters_total == i2["qp_iters_total"][b], (b, oi2.qp_iters_total, i2["qp_iters_total"][b])
        assert abs(sT2[b] - T2) <= 1e-6 * T2 and np.abs(sx2[b] - xs2).max() <= 1e-5 and oi2.status == i2["status"][b]
    # the plain solve call's default stays OFF: flags 0 = cold QPs from lambda = 0, whatever the slot's previous solve left behind
    s0 = M.Solver(M.default_config(nseg, 2, margins=MARGINS), B)
    a = s0.solve(x0, xf, (wx, wu, wT)); b_ = s0.solve(x0, xf, (wx, wu, wT))
    assert np.array_equal(a[0], b_[0]) and np.array_equal(a[3]["qp_iters_total"], b_[3]["qp_iters_total"])
    ocold = o.default_config(nseg, 2, margins=MARGINS)
    assert a[3]["qp_iters_total"][0] == o.solve(ocold, x0[0], xf[0], wx[0], wu[0], wT[0])[3].qp_iters_total


def test_receding_horizon_arrival_vs_oracle(M):
    """arrival (include/mpcmp.h, mpcmp_rh_run): control periods so long that every instance arrives within a few re-solves.  The oracle chain with the
    same rule retires the same instances in the same steps: equal states, final times, ADMM iteration counts of the last solve executed, ARRIVED
    bits and re-solve counts, eager and graph replay; a retired instance keeps its state and record while the others go on"""
    cfg, ocfg = M.default_config(4, 2, margins=MARGINS), o.default_config(4, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1)
    from mpc_motion_planner_amd import scenarios
    B, dt = 6, 0.4
    x0, xf = scenarios.make_batch(B, stream_offset=900)
    for steps in (3, 10):
        xr, Tr, its, st, ret, ns = _oracle_rh_chain(ocfg, x0, xf, steps, dt)
        assert ret.any() and (steps == 3 and not ret.all() or steps == 10 and ret.all())
        for use_graph in (False, True):
            s = M.Solver(cfg, B)
            s.rh_init(x0, xf)
            s.rh_run(steps, dt, use_graph=use_graph)
            xg, sx, su, sT, info = s.rh_get()
            assert np.array_equal((info["status"] & M.STATUS_ARRIVED) != 0, ret), (steps, use_graph, info["status"], ret)
            assert np.array_equal(info["status"] & 63, st) and np.array_equal(info["qp_iters_total"], its)
            assert np.abs(xg - xr).max() < 1e-6 and np.abs(sT - Tr).max() < 1e-6 * np.abs(Tr).max()
            assert s.rh_stats() == (ns, int(ret.sum()))
            if steps == 10:      # everybody has arrived: further steps change nothing and solve nothing
                s.rh_run(3, dt, use_graph=use_graph)
                assert np.array_equal(s.rh_get()[0], xg) and s.rh_stats() == (ns, B)
                assert np.abs(xg - xf).max() <= cfg.eps_target + 1e-9 or np.all(sT <= dt)


def test_failed_solve_holds_state_and_restarts_vs_oracle(M):
    """the hard bits of the FINAL iterate (T outside its box, NaN) exist only in the record k_step writes; they are now written back to the
    workspace status the next k_init / k_advance read.  A final-time box too narrow for most instances ([0, 1.5] s) makes their solves end with
    MPCMP_STATUS_T_OUT_OF_BOX: such an instance holds its state, re-solves from the built-in guess and carries no multipliers — the oracle chain
    does the same (orc_solve_carry zeroes lam_io, the chain restarts): equal states, iteration counts and status words after every step count"""
    kw = dict(lbT=0.0, ubT=1.5)
    cfg, ocfg = M.default_config(4, 2, margins=MARGINS, **kw), o.default_config(4, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1, **kw)
    from mpc_motion_planner_amd import scenarios
    B, dt = 6, 0.05
    x0, xf = scenarios.make_batch(B, stream_offset=900)
    saw_held = False
    for steps in (1, 2, 4):
        xr, Tr, its, st, ret, ns = _oracle_rh_chain(ocfg, x0, xf, steps, dt)
        s = M.Solver(cfg, B)
        s.rh_init(x0, xf)
        s.rh_run(steps, dt, use_graph=(steps == 4))
        xg, sx, su, sT, info = s.rh_get()
        assert np.array_equal(info["status"] & 63, st), (steps, info["status"], st)
        assert np.array_equal(info["qp_iters_total"], its), (steps, info["qp_iters_total"], its)
        assert np.abs(xg - xr).max() < 1e-6
        if steps == 1:
            bad = (st & 32) != 0
            assert bad.any() and not bad.all()
            assert np.array_equal(xg[bad], x0[bad])           # held: there is no trajectory to follow
            saw_held = True
    assert saw_held


def test_receding_horizon_full_length_no_hard_failure(M):
    """configs[4] in full: 512 instances x 200 re-solves of 10 ms with the driver's defaults (carried multipliers, warm QP duals, arrival).  Most
    instances arrive; NO instance ends in a hard failure, with a NaN or with T outside its box, every state is finite, the arrived ones sit where
    their plan ended, the live re-solve count is what the arrivals leave, and the run is bitwise repeatable"""
    cfg = M.default_config(4, 2, margins=MARGINS)
    from mpc_motion_planner_amd import scenarios
    B, steps = 512, 200
    x0, xf = scenarios.make_batch(B, MARGINS)
    s = M.Solver(cfg, B)
    outs = []
    for rep in range(2):
        s.rh_init(x0, xf)
        s.rh_run(steps, 0.01, use_graph=True)
        xg, sx, su, sT, info = s.rh_get()
        done, arrived = s.rh_stats()
        outs.append((xg.copy(), info["status"].copy(), done, arrived))
        assert np.all(np.isfinite(xg)) and np.all(np.isfinite(sT))
        assert np.all((info["status"] & 7) == 0), np.flatnonzero(info["status"] & 7)[:8]
        assert ((info["status"] & M.STATUS_T_OUT_OF_BOX) != 0).mean() <= 0.01, np.flatnonzero(info["status"] & 32)[:8]      # (transient: such an instance restarts)
        arr = (info["status"] & M.STATUS_ARRIVED) != 0
        assert arrived == int(arr.sum()) and arrived > B // 16
        assert B <= done < B * steps and done >= B * steps - arrived * steps
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2:] == outs[1][2:]


def test_more_than_255_capped_qps_are_counted(M):
    """mpcmp_info.qp_capped used to live in eight bits of the status word and wrapped at 256: 300 SQP iterations of a QP capped at ONE
    ADMM iteration each — every QP is capped — are counted as 300, the QP_CAPPED bit stays set, and the oracle reports the same record"""
    cfg, ocfg = _cfgs(M, 1, 300, qp_iters=1, check_every=1)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(2, stream_offset=61)
    s = M.Solver(cfg, 2)
    wx, wu, wT = s.warm_start(x0, xf)
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    assert np.all(info["qp_capped"] == 300) and np.all(info["status"] & 8) and np.all(info["qp_iters_total"] == 300)
    for b in range(2):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert oi.qp_capped == 300 and oi.status == info["status"][b] and abs(sT[b] - T) <= 1e-6 * abs(T)


def test_traj_stats_vs_oracle(M):
    """examples/benchmark.cpp:58-160: extrema, terminal error and the four pass flags of a resampled trajectory"""
    cfg, ocfg = _cfgs(M, 4, 3)
    from mpc_motion_planner_amd import scenarios
    B = 5
    x0, xf = scenarios.make_batch(B, stream_offset=11)
    s = M.Solver(cfg, B)
    sx, su, sT, _ = s.solve(x0, xf)
    su2 = su.copy(); su2[0, 3] = 1e5                # force a jerk failure in problem 0
    sx2 = sx.copy(); sx2[1, :, 1] = 2.5; sx2[1, :, 3] = -0.1; sx2[1, :, 5] = 0.2   # arm pitched below the table: collision
    for (X, U) in ((sx, su), (sx2, su2)):
        out = s.traj_stats(X, U, sT, xf, n_pts=200)
        for b in range(B):
            ref = o.traj_stats(4, X[b], U[b], sT[b], xf[b], 200)
            assert np.array_equal(out[b, 70:], ref[70:]), (b, out[b, 70:], ref[70:])
            assert np.abs(out[b, :70] - ref[:70]).max() < 1e-8 * (1 + np.abs(ref[:70]).max())
    out = s.traj_stats(sx2, su2, sT, xf)
    assert out[0, 70] == 0.0 and out[1, 73] == 0.0


def test_cpp_examples_run(M, tmp_path):
    """the C++ MotionPlanner mirror end to end: offline_trajectory (403 x 29) and the batched benchmark (162 columns)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("offline_trajectory", "benchmark"):
        exe = str(tmp_path / name)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"),
                               os.path.join(root, "examples", name + ".cpp"), "-L" + os.path.join(root, "mpc_motion_planner_amd"),
                               "-lmpcmp", "-Wl,-rpath," + os.path.join(root, "mpc_motion_planner_amd"), "-o", exe])
    out1 = str(tmp_path / "optimal_solution.txt")
    subprocess.check_call([str(tmp_path / "offline_trajectory"), "", out1, "7"])
    d = np.loadtxt(out1)
    assert d.shape == (403, 29)                       # examples/offline_trajectory.cpp:69-105
    assert abs(d[1, 0]) < 1e-12 and abs(d[202, 0]) < 1e-12 and d[402, 0] > 0.3
    assert np.abs(d[402, 1:15] - d[0, 1:15]).max() < 5e-2      # MPC trajectory ends at the target
    out2 = str(tmp_path / "benchmark_data.txt")
    subprocess.check_call([str(tmp_path / "benchmark"), "", out2, "24"])
    b = np.loadtxt(out2)
    assert b.shape == (24, 162)                       # analysis/benchmark_analysis.ipynb cell 1
    assert set(np.unique(b[:, 140:148])) <= {0.0, 1.0}


def test_edge_cases(M):
    """single problem, full-capacity batch, coincident start/target, non-finite input (flagged, not fatal)"""
    cfg, ocfg = _cfgs(M, 4, 2)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(7, stream_offset=300)
    s = M.Solver(cfg, 7)
    sx7, su7, sT7, info7 = s.solve(x0, xf)                         # exactly max_batch
    sx1, su1, sT1, info1 = s.solve(x0[3:4], xf[3:4])               # a single problem
    assert np.array_equal(sx1[0], sx7[3]) and sT1[0] == sT7[3]
    # start == target: the minimum-time problem degenerates; the solver must return finite numbers
    sxe, sue, sTe, infoe = s.solve(x0[:2], x0[:2])
    assert np.all(np.isfinite(sTe)) and np.all((infoe["status"] & 7) == 0) and np.all(sTe < sT7[:2])
    # non-finite start state: reported through status bit 0 for that problem only
    bad = x0.copy(); bad[2, 0] = np.nan
    _, _, sTb, infob = s.solve(bad, xf)
    assert infob["status"][2] & 1 and np.all((infob["status"][[0, 1, 3, 4, 5, 6]] & 7) == 0)
    assert np.array_equal(sTb[[0, 1, 3, 4, 5, 6]], sT7[[0, 1, 3, 4, 5, 6]])
    # the oracle agrees on the degenerate case
    xg, ug, Tg = o.warm_start(ocfg, x0[0], x0[0])
    xs, us, T, oi = o.solve(ocfg, x0[0], x0[0], xg, ug, Tg)
    assert abs(sTe[0] - T) <= 1e-6 * max(T, 1e-3) + 1e-9


def test_headline_configuration_full_size(M):
    """BASELINE.json configs[1] at full size (1024 problems, N=13, 20 SQP iterations): size-independent properties
    (every problem reported ok, bitwise reproducible although the launch order of the QP kernel is data dependent,
    a problem's result does not depend on the batch it travels in) and oracle parity on a sample."""
    cfg, ocfg = _cfgs(M, 4, 20)
    from mpc_motion_planner_amd import scenarios
    B = 1024
    x0, xf = scenarios.make_batch(B)
    s = M.Solver(cfg, B)
    sx, su, sT, info = s.solve(x0, xf)
    assert np.all((info["status"] & 7) == 0) and np.all(np.isfinite(sx)) and np.all(np.isfinite(sT))
    assert np.all(info["sqp_iters"] == 20) and np.all(info["qp_iters_total"] <= 20 * 700)
    # the SQP of the reference has no safeguard beyond its line search: a few hard problems end far from feasibility
    # (one of this batch even with T < 0).  The oracle fails on them in exactly the same way (checked below).
    assert (sT > 0).mean() >= 0.99 and np.median(info["term_err_inf"]) < 2e-2
    # ... and every such problem is FLAGGED in its record (include/mpcmp.h MPCMP_STATUS_*): T outside [lbT, ubT] -> bit 32; an iterate outside
    # the tolerances (defect / path violation > eps_abs, terminal error > eps_target + eps_abs) -> bit 16; a QP that hit qp_iters -> bit 8
    outside = (info["defect_inf"] > cfg.eps_abs) | (info["path_viol_inf"] > cfg.eps_abs) | (info["term_err_inf"] > cfg.eps_target + cfg.eps_abs)
    assert np.array_equal((info["status"] & 16) != 0, outside)
    assert np.array_equal((info["status"] & 32) != 0, (sT < cfg.lbT - 1e-9) | (sT > cfg.ubT + 1e-9)) and np.all((info["status"][sT < 0] & 32) != 0)
    assert np.array_equal((info["status"] & 8) != 0, info["qp_capped"] > 0) and np.all(info["qp_capped"] <= 20)
    assert np.all((info["status"] == 0) == (~outside & (info["qp_capped"] == 0) & (sT >= cfg.lbT - 1e-9) & (sT <= cfg.ubT + 1e-9)))
    sx2, su2, sT2, info2 = s.solve(x0, xf)
    assert np.array_equal(sx, sx2) and np.array_equal(su, su2) and np.array_equal(sT, sT2)
    assert np.array_equal(info["qp_iters_total"], info2["qp_iters_total"])
    sub = np.arange(100, 164)                                     # the same problems as a small batch of their own
    sxs, _, sTs, _ = s.solve(x0[sub], xf[sub])
    assert np.array_equal(sTs, sT[sub]) and np.array_equal(sxs, sx[sub])
    for b in (0, 333, 1023, int(np.argmin(sT))):
        wx, wu, wT = o.warm_start(ocfg, x0[b], xf[b])
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx, wu, wT)
        assert abs(sT[b] - T) <= 1e-6 * abs(T) and np.abs(sx[b] - xs).max() <= 1e-6 and np.abs(su[b] - us).max() <= 1e-5
        assert info["qp_iters_total"][b] == oi.qp_iters_total


@pytest.mark.parametrize("nseg,sqp", [(4, 3), (6, 2)])
def test_ragged_batch_sizes_around_the_two_stream_split(M, nseg, sqp):
    """a batch of 512 problems or more is solved as parts on several streams (mpcmp.hip: solve_impl): sizes that do not split evenly (513, 1023, 1025), the
    thresholds themselves and one below (511, 512; 1023, 1024: the N = 13 path takes three parts from 1024 on), a single problem, and a context used below its capacity — every problem's result is the one it has
    in the full batch, bit for bit, whatever the split it travels in (N = 13: k_qp2, N = 19: k_qp3f + k_qp5)"""
    cfg, _ = _cfgs(M, nseg, sqp)
    from mpc_motion_planner_amd import scenarios
    Bmax = 1025                                                    # (N = 13: three parts from 1024 problems on, two below)
    x0, xf = scenarios.make_batch(Bmax, stream_offset=5000)
    s = M.Solver(cfg, 1025)
    sx, su, sT, info = s.solve(x0, xf)
    assert np.all((info["status"] & 7) == 0) and np.all(np.isfinite(sx))
    for B in (1, 511, 512, 513, 1023, 1024):
        sxb, sub, sTb, ib = s.solve(x0[:B], xf[:B])
        assert np.array_equal(sTb, sT[:B]) and np.array_equal(sxb, sx[:B]) and np.array_equal(sub, su[:B]), B
        assert np.array_equal(ib["qp_iters_total"], info["qp_iters_total"][:B]) and np.array_equal(ib["status"], info["status"][:B])
    off = 700                                                      # the tail of the batch as a batch of its own: other slots, other part
    sxt, _, sTt, it = s.solve(x0[off:], xf[off:])
    assert np.array_equal(sTt, sT[off:]) and np.array_equal(sxt, sx[off:]) and np.array_equal(it["qp_iters_total"], info["qp_iters_total"][off:])


def test_reference_as_shipped_configuration_full_size(M):
    """BASELINE.json configs[0] depth at batch size (1024 problems, N = 19, 2 SQP iterations: robot_ocp.hpp:32, motionPlanner.cpp:15) from
    the jerk-limited warm start, through k_qp3f (Schur products on the matrix cores) + k_qp3: every problem reported ok, bitwise
    reproducible, independent of the batch a problem travels in, and oracle parity on a sample."""
    cfg, ocfg = _cfgs(M, 6, 2)
    from mpc_motion_planner_amd import scenarios
    lim = M.default_limits()
    margins = (0.9, 0.9, 0.5, 0.9)
    vmax, amax, jmax = margins[1] * lim["vmax"], margins[2] * lim["amax"], 0.1 * lim["jmax"]
    B = 1024
    x0, xf = scenarios.make_batch(B)
    s = M.Solver(cfg, B)
    warm = s.warm_start_jerk(x0, xf, jmax)
    sx, su, sT, info = s.solve(x0, xf, warm)
    assert np.all((info["status"] & 7) == 0) and np.all(np.isfinite(sx)) and np.all(np.isfinite(su)) and np.all(np.isfinite(sT))
    assert np.all(info["sqp_iters"] == 2) and np.all(info["qp_iters_total"] <= 2 * 700) and np.all(info["qp_iters_total"] >= 2 * 25)
    assert (sT > 0).mean() >= 0.99
    sx2, su2, sT2, info2 = s.solve(x0, xf, warm)
    assert np.array_equal(sx, sx2) and np.array_equal(su, su2) and np.array_equal(sT, sT2)
    assert np.array_equal(info["qp_iters_total"], info2["qp_iters_total"])
    sub = np.arange(700, 764)                                     # the same problems as a small batch of their own
    sxs, _, sTs, _ = s.solve(x0[sub], xf[sub], tuple(w[sub] for w in warm))
    assert np.array_equal(sTs, sT[sub]) and np.array_equal(sxs, sx[sub])
    for b in (0, 511, 512, 1023):
        xg, ug, Tg = o.warm_start_jerk(6, vmax, amax, jmax, x0[b], xf[b])
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], xg, ug, Tg)
        assert abs(sT[b] - T) <= 1e-6 * abs(T) and np.abs(sx[b] - xs).max() <= 1e-6 and np.abs(su[b] - us).max() <= 1e-5
        assert info["qp_iters_total"][b] == oi.qp_iters_total


def test_jerk_limited_warm_start_vs_oracle_and_stored_ruckig(M, golden_dir):
    """the generator that stands in for Ruckig (motionPlanner.cpp:146-175): HIP kernel vs the oracle's restatement on random
    state pairs, vs the reference's stored Ruckig trajectory, and as the warm start of a solve"""
    import json, os
    lim = M.default_limits()
    margins = (0.9, 0.9, 0.5, 0.9)
    cfg, ocfg = _cfgs(M, 4, 2)
    vmax, amax, jmax = margins[1] * lim["vmax"], margins[2] * lim["amax"], 0.1 * lim["jmax"]
    from mpc_motion_planner_amd import scenarios
    B = 64
    x0, xf = scenarios.make_batch(B, stream_offset=700)
    s = M.Solver(cfg, B)
    wx, wu, wT = s.warm_start_jerk(x0, xf, jmax)
    out, T = s.jerk_trajectory(x0, xf, jmax, 100)
    for b in range(B):
        xg, ug, Tg = o.warm_start_jerk(4, vmax, amax, jmax, x0[b], xf[b])
        assert abs(wT[b] - Tg) <= 1e-9 * Tg and abs(T[b] - Tg) <= 1e-9 * Tg
        assert np.abs(wx[b] - xg).max() <= 1e-8 and np.abs(wu[b] - ug).max() <= 1e-6
        oo, _ = o.jerk_trajectory(vmax, amax, jmax, x0[b], xf[b], 100)
        assert np.abs(out[b][:, :15] - oo[:, :15]).max() <= 1e-8
    assert np.all(np.abs(out[:, :, 8:15]) <= vmax + 1e-9)
    # non-zero boundary accelerations (set_current_state / set_target_state forward them to Ruckig, motionPlanner.cpp:36-38,50-52): HIP vs oracle on
    # random accelerations, both boundary states met in q, qd AND qdd, and zero accelerations through the *_acc_* entry points = the plain ones bit for bit
    rng = np.random.default_rng(5)
    a0, aT = rng.uniform(-0.8, 0.8, (B, 7)) * amax, rng.uniform(-0.8, 0.8, (B, 7)) * amax
    x0s = x0.copy(); xfs = xf.copy(); x0s[:, 7:] *= 0.6; xfs[:, 7:] *= 0.6
    wxa, wua, wTa = s.warm_start_jerk(x0s, xfs, jmax, acc0=a0, accT=aT)
    outa, Ta = s.jerk_trajectory(x0s, xfs, jmax, 100, acc0=a0, accT=aT)
    pta, _ = s.jerk_point(x0s, xfs, jmax, 0.37 * Ta, acc0=a0, accT=aT)
    for b in range(B):
        xg, ug, Tg = o.warm_start_jerk(4, vmax, amax, jmax, x0s[b], xfs[b], acc0=a0[b], accT=aT[b])
        assert abs(wTa[b] - Tg) <= 1e-9 * Tg and abs(Ta[b] - Tg) <= 1e-9 * Tg
        assert np.abs(wxa[b] - xg).max() <= 1e-8 and np.abs(wua[b] - ug).max() <= 1e-6
        oo, _ = o.jerk_trajectory(vmax, amax, jmax, x0s[b], xfs[b], 100, acc0=a0[b], accT=aT[b])
        assert np.abs(outa[b] - oo).max() <= 1e-6
        assert np.abs(outa[b][0, 15:22] - a0[b]).max() <= 1e-9 and np.abs(outa[b][-1, 15:22] - aT[b]).max() <= 1e-8
        assert np.abs(outa[b][-1, 1:8] - xfs[b][:7]).max() <= 1e-8 and np.abs(outa[b][-1, 8:15] - xfs[b][7:]).max() <= 1e-8
        assert np.abs(pta[b][:21] - np.array([np.interp(0.37 * Ta[b], oo[:, 0], oo[:, c]) for c in range(1, 22)])).max() < 5e-2     # (the point entry sees the same trajectory)
    z = np.zeros((B, 7))
    wxz, wuz, wTz = s.warm_start_jerk(x0, xf, jmax, acc0=z, accT=z)
    assert np.array_equal(wxz, wx) and np.array_equal(wuz, wu) and np.array_equal(wTz, wT)
    # limits given by the caller (ruckig's input.max_velocity / max_acceleration, motionPlanner.cpp:86-88,149) instead of the context's bounds:
    # HIP vs oracle with tighter limits; the context's own limits passed explicitly = the plain entry point bit for bit; a limit <= 0 is EINVAL
    wxl, wul, wTl = s.warm_start_jerk(x0s, xfs, jmax, acc0=a0, accT=aT, vmax=0.8 * vmax, amax=0.9 * amax)
    ptl, Tl = s.jerk_point(x0s, xfs, jmax, 0.4 * wTl, acc0=a0, accT=aT, vmax=0.8 * vmax, amax=0.9 * amax)
    for b in range(B):
        xg, ug, Tg = o.warm_start_jerk(4, 0.8 * vmax, 0.9 * amax, jmax, x0s[b], xfs[b], acc0=a0[b], accT=aT[b])
        assert abs(wTl[b] - Tg) <= 1e-9 * Tg and abs(Tl[b] - Tg) <= 1e-9 * Tg
        assert np.abs(wxl[b] - xg).max() <= 1e-8 and np.abs(wul[b] - ug).max() <= 1e-6
    wxe, wue, wTe = s.warm_start_jerk(x0, xf, jmax, vmax=vmax, amax=amax)
    assert np.array_equal(wxe, wx) and np.array_equal(wue, wu) and np.array_equal(wTe, wT)
    with pytest.raises(Exception):
        s.warm_start_jerk(x0, xf, jmax, vmax=0.0 * vmax)
    # a boundary acceleration that cannot be brought to zero inside the velocity limit (v0 + a0 |a0| / 2J > vmax) is rejected (MPCMP_EINVAL,
    # as Ruckig's ErrorInvalidInput), by all three host entry points; the same acceleration at a slower start is accepted
    xv = x0s[:1].copy(); xv[0, 7:] = 0.999 * vmax; av = amax[None].copy()
    for call in (lambda: s.warm_start_jerk(xv, xfs[:1], jmax, acc0=av), lambda: s.jerk_trajectory(xv, xfs[:1], jmax, 10, acc0=av),
                 lambda: s.jerk_point(xv, xfs[:1], jmax, np.array([0.1]), acc0=av), lambda: s.warm_start_jerk(xfs[:1], xv, jmax, accT=-av)):
        with pytest.raises(M.MpcmpError):
            call()
    xv[0, 7:] = 0.9 * vmax
    s.warm_start_jerk(xv, xfs[:1], jmax, acc0=av)
    # KAT-RK through the GPU path (6 stored digits)
    g = json.load(open(os.path.join(golden_dir, "gold_traj.json")))
    k0 = np.concatenate([g["q0"], g["v0"]])[None]; kf = np.concatenate([g["qT"], g["vT"]])[None]
    ko, kT = s.jerk_trajectory(k0, kf, jmax, 200)
    assert abs(kT[0] - g["T_ruckig"]) < 2e-6 and np.abs(ko[0][:, 1:8] - np.array(g["q_rk"])).max() < 2e-5
    # as warm start of the solve (the reference's solve_trajectory(true)): same result as the oracle from the same guess
    sx, su, sT, info = s.solve(x0[:4], xf[:4], (wx[:4], wu[:4], wT[:4]))
    for b in range(4):
        xs, us, Tb, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert abs(sT[b] - Tb) <= 1e-6 * abs(Tb) and np.abs(sx[b] - xs).max() <= 1e-6 and info["qp_iters_total"][b] == oi.qp_iters_total


def test_host_staging_across_a_scratch_growth_and_optional_arrays(M):
    """the host-pointer entry points stage their arrays in one device scratch of the context that grows when a call needs more than it holds (1 MiB at
    first): results before, during and after a growth, and every combination of optional arrays, all bit for bit (same kernels, same inputs; no solve)"""
    import torch
    from mpc_motion_planner_amd import scenarios
    cfg, _ = _cfgs(M, 4, 1)
    B = 2
    s = M.Solver(cfg, 8)
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    x0, xf = scenarios.make_batch(B, stream_offset=900)
    wx, wu, wT = s.warm_start_jerk(x0, xf, jmax)
    rng = np.random.default_rng(11)
    q, v, a = rng.uniform(-2, 2, (3, 7)), rng.uniform(-2, 2, (3, 7)), rng.uniform(-10, 10, (3, 7))
    # 1. inside the first allocation
    tau1, smp1 = s.rnea(q, v, a), s.sample(wx, wu, wT, n_pts=8)
    assert np.all(np.isfinite(tau1)) and np.all(np.isfinite(smp1)) and np.abs(tau1).max() > 0.0
    # 2. the output alone (2 x 3001 x 29 doubles = 1.39 MB) is larger than the first allocation: the scratch grows in this call
    big = s.sample(wx, wu, wT, n_pts=3000)
    tx, tu, tT = (torch.from_numpy(np.ascontiguousarray(w)).to("cuda") for w in (wx, wu, wT))
    tout = torch.zeros(B, 3001, 29, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.sample_device(B, tx.data_ptr(), tu.data_ptr(), tT.data_ptr(), 3000, tout.data_ptr())
    torch.cuda.synchronize()
    assert big.shape == (B, 3001, 29) and np.array_equal(big, tout.cpu().numpy())
    # 3. after the growth
    assert np.array_equal(s.rnea(q, v, a), tau1) and np.array_equal(s.sample(wx, wu, wT, n_pts=8), smp1)
    # 4. optional inputs of rh_update: rh_get shows the states (the targets are not among its outputs); a row is written only where x is given
    s.rh_init(x0, xf)
    xa, xb = x0 + 0.01, x0 - 0.02
    s.rh_update([1], x=xa[1:])
    assert np.array_equal(s.rh_get()[0], np.stack([x0[0], xa[1]]))
    s.rh_update([0], xf=xf[1:])
    assert np.array_equal(s.rh_get()[0], np.stack([x0[0], xa[1]]))
    s.rh_update(x=xb, xf=xf[::-1])
    assert np.array_equal(s.rh_get()[0], xb)
    # 5. optional inputs of jerk_point: a boundary acceleration that is not given is zero
    x0s, xfs = x0.copy(), xf.copy(); x0s[:, 7:] *= 0.6; xfs[:, 7:] *= 0.6
    acc, z, t = rng.uniform(-0.8, 0.8, (B, 7)) * MARGINS[2] * M.default_limits()["amax"], np.zeros((B, 7)), 0.4 * wT
    for only, full in ((dict(acc0=acc), dict(acc0=acc, accT=z)), (dict(accT=acc), dict(acc0=z, accT=acc))):
        p1, T1 = s.jerk_point(x0s, xfs, jmax, t, **only)
        p2, T2 = s.jerk_point(x0s, xfs, jmax, t, **full)
        assert np.array_equal(p1, p2) and np.array_equal(T1, T2) and np.all(np.isfinite(p1))
