"""Via-point routes on the GPU (include/mpcmp.h, "via-point routes").  The leg builder, the join, the route sampler and the argument checks against
NumPy restatements written here and in test_routes_host.py; the route solve against the plain solve of its legs in a fresh context, bit for bit, on
the three kernel paths (k_qp2 at N = 7, k_qp5 at N = 19, k_qp3 with two arms at N = 19), which ties the feature to the existing oracle parity without
a tolerance of its own."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as o
from test_gpu_receding_horizon import MARGINS, dual_states
from test_routes_host import chord_np, locate_np

pytestmark = pytest.mark.gpu

BAD = 1 | 2 | 4 | 16 | 32          # the inadmissible set of mpcmp_select_clear_batch: NAN, NOT_PD, XCH_DEAD, OUTSIDE_TOL, T_OUT_OF_BOX
MS = (0, 1, 3)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _jmax(M):
    return MARGINS[4] * M.default_limits()["jmax"]


def _solver(M, nseg, sqp, narm=1, max_batch=12, **kw):
    cfg = M.default_config(nseg, sqp, margins=MARGINS, **kw)
    return M.Solver(cfg, max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)


def _states(narm, B, off=0):
    from mpc_motion_planner_amd import scenarios
    return dual_states(B, off) if narm == 2 else scenarios.make_batch(B, MARGINS, stream_offset=off)


def _vias(M, x0, xf, nvia, narm, seed=3, spread=0.25):
    """the midpoint of start and target plus a seeded offset, kept inside the position margins"""
    cfg = M.default_config(2, 1, margins=MARGINS)
    lo, hi = np.tile(np.array(cfg.lbx[:7]), narm), np.tile(np.array(cfg.ubx[:7]), narm)
    nq = 7 * narm
    r = np.random.default_rng(seed)
    f = (np.arange(nvia) + 1.0) / (nvia + 1.0)
    via = x0[:, None, :nq] + f[None, :, None] * (xf[:, None, :nq] - x0[:, None, :nq]) + r.uniform(-spread, spread, (x0.shape[0], nvia, nq))
    return np.ascontiguousarray(np.clip(via, lo + 0.05, hi - 0.05))


# ---- restatements ----
def legs_np(x0, via, xf, rows, narm, speed, via_qd=None):
    B, nvia, nq = via.shape
    P = np.concatenate([x0[:, None, :nq], via, xf[:, None, :nq]], axis=1)
    V = np.zeros_like(P); V[:, 0] = x0[:, nq:]; V[:, -1] = xf[:, nq:]
    for b in range(B):
        for i in range(1, nvia + 1):
            row = rows[b * (nvia + 1) + i] if rows.ndim else rows
            V[b, i] = via_qd[b, i - 1] if via_qd is not None else chord_np(P[b, i - 1], P[b, i], P[b, i + 1], row, narm, speed[b])
    l0 = np.concatenate([P[:, :-1], V[:, :-1]], axis=2).reshape(B * (nvia + 1), 2 * nq)
    lf = np.concatenate([P[:, 1:], V[:, 1:]], axis=2).reshape(B * (nvia + 1), 2 * nq)
    return l0, lf, V[:, 1:-1]


def _nmax(m, v):
    return v if (v > m or v != v) else m


def _nmin(m, v):
    return v if (v < m or v != v) else m


def join_np(M, sx, su, sT, info, clr=None):
    """the join of include/mpcmp.h: sequential in leg order; maxima and minima keep a NaN"""
    B, nl = sT.shape
    rT, rinfo, seam = np.zeros(B), np.zeros(B, dtype=M.INFO_DTYPE), np.zeros(B, dtype=M.ROUTE_SEAM_DTYPE)
    rclr = np.zeros(B, dtype=M.CLEARANCE_DTYPE)
    for b in range(B):
        r = info[b, 0].copy(); T = sT[b, 0]; Tl = sT[b, 0]; longest = 0; sj = aj = 0.0
        bad = 0 if info[b, 0]["status"] & BAD else -1
        for m in range(1, nl):
            i = info[b, m]
            T = T + sT[b, m]
            for k in ("viol_l1", "defect_inf", "path_viol_inf", "term_err_inf"):
                r[k] = _nmax(r[k], i[k])
            r["last_alpha"] = _nmin(r["last_alpha"], i["last_alpha"])
            r["sqp_iters"] = max(r["sqp_iters"], i["sqp_iters"])
            r["qp_iters_total"] += i["qp_iters_total"]; r["qp_capped"] += i["qp_capped"]; r["status"] |= i["status"]
            if sT[b, m] > Tl:
                Tl, longest = sT[b, m], m
            if bad < 0 and i["status"] & BAD:
                bad = m
            for v in np.abs(sx[b, m - 1, -1] - sx[b, m, 0]):
                sj = _nmax(sj, v)
            for v in np.abs(su[b, m - 1, -1] - su[b, m, 0]):
                aj = _nmax(aj, v)
        r["T"] = T; rT[b] = T; rinfo[b] = r
        seam[b] = (sj, aj, longest, bad)
        if clr is None:
            continue
        d, tm, tf, sp, ot, nh, st, E = np.inf, -1.0, -1.0, -1, 0, 0, 0, 0.0
        for m in range(nl):
            c = clr[b, m]
            st |= c["status"]; nh += c["n_hit"]
            if c["sphere"] >= 0 and c["d_min"] < d:
                d, tm, sp, ot = c["d_min"], c["t_min"] + E, c["sphere"], c["other"]
            if tf < 0 and c["t_first"] >= 0:
                tf = c["t_first"] + E
            E = E + sT[b, m]
        if st & M.CLR_NAN:
            d, tm, tf, sp, ot, nh = np.nan, -1.0, -1.0, -1, 0, 0
        rclr[b] = (d, tm, tf, sp, ot, nh, st)
    return rT, rinfo, seam, rclr


def select_np(T, info, clr, group, n_groups):
    chosen = np.full(n_groups, -1, dtype=np.int32)
    for g in range(n_groups):
        best = None
        for i in np.nonzero(group == g)[0]:
            if (info[i]["status"] & BAD) == 0 and clr[i]["status"] == 0 and (best is None or T[i] < T[best]):
                best = i
        chosen[g] = -1 if best is None else best
    return chosen


def row_np(nseg, xs, us, tau, model=None):
    """q, qd, qdd, tau of one trajectory at the normalised time tau: the Lagrange interpolation on the segment of oracle_py.sample, the oracle's RNEA"""
    xi = np.array([-1.0, -0.5, 0.5, 1.0])
    s = min(max(int(np.floor(tau * nseg)), 0), nseg - 1)
    xx = 2.0 * (tau * nseg - s) - 1.0
    Lg = np.array([np.prod([(xx - xi[k]) / (xi[j] - xi[k]) for k in range(4) if k != j]) for j in range(4)])
    x = Lg @ xs[3 * s:3 * s + 4]; u = Lg @ us[3 * s:3 * s + 4]
    return np.concatenate([x[:7], x[7:], u, o.rnea(x[:7], x[7:], u, model)])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. leg builder --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm,nseg", [(1, 2), (2, 6)])
def test_leg_builder_matches_its_restatement(M, narm, nseg):
    s = _solver(M, nseg, 1, narm)
    B = 3
    x0, xf = _states(narm, B)
    cfg_row = M.bounds_from_config(s.cfg)
    speed = np.array([1.0, 0.5, 0.0])
    close = lambda a, r: np.all(np.abs(a - r) <= 1e-13 * np.abs(r))
    for nvia in MS:
        via = _vias(M, x0, xf, nvia, narm)
        for sp in (None, speed):
            l0, lf, vq = s.route_legs(x0, via, xf, speed=sp)
            r0, rf, rv = legs_np(x0, via, xf, cfg_row, narm, np.ones(B) if sp is None else sp)
            assert close(l0, r0) and close(lf, rf) and close(vq, rv), (nvia, sp)
            assert np.array_equal(l0[:, :7 * narm], r0[:, :7 * narm]) and np.array_equal(lf[:, :7 * narm], rf[:, :7 * narm])      # positions are copies
            if nvia:
                assert np.array_equal(l0.reshape(B, nvia + 1, -1)[:, 1:], lf.reshape(B, nvia + 1, -1)[:, :-1])       # a leg starts where the one before ends
                assert sp is None or np.all(vq[2] == 0)
                assert np.any(vq[0] != 0)
        if nvia == 0:
            assert np.array_equal(l0, x0) and np.array_equal(lf, xf)
            continue
        # a given via velocity is copied bit for bit
        given = np.random.default_rng(5).uniform(-0.3, 0.3, via.shape)
        l0, lf, vq = s.route_legs(x0, via, xf, via_qd=given)
        r0, rf, _ = legs_np(x0, via, xf, cfg_row, narm, np.ones(B), via_qd=given)
        assert same_bits(vq, given) and np.array_equal(l0, r0) and np.array_equal(lf, rf)
    # bound rows: the via reads the row of the leg slot that STARTS there.  Route 0 with one via: leg slot 0 ends at it, leg slot 1 starts at it
    nvia = 1
    via = _vias(M, x0, xf, nvia, narm)
    rows = s.bounds_table(n=B * (nvia + 1))
    rows["ubx"][0, 7:] *= 0.01; rows["lbx"][0, 7:] *= 0.01        # slot 0: a velocity box a hundred times narrower
    rows["ubx"][1, 7:] *= 0.5; rows["lbx"][1, 7:] *= 0.5          # slot 1: half the box
    s.set_bounds(rows)
    _, _, vq = s.route_legs(x0, via, xf)
    _, _, rv = legs_np(x0, via, xf, rows, narm, np.ones(B))
    assert close(vq, rv)
    swapped = rows.copy(); swapped[[0, 1]] = rows[[1, 0]]
    _, _, wrong = legs_np(x0, via, xf, swapped, narm, np.ones(B))
    assert not close(vq[0], wrong[0])                              # the row of the leg that ENDS there would give another velocity
    assert np.all(np.abs(vq[0, 0]) <= np.tile(rows["ubx"][1, 7:], narm))
    s.clear_bounds()
    _, _, vq = s.route_legs(x0, via, xf)
    assert close(vq, legs_np(x0, via, xf, cfg_row, narm, np.ones(B))[2])


# ---- 2. the route solve = the plain solve of its legs --------------------------------------------------------------------------------------
def _plain_legs_device(M, s2, l0, lf, jmax):
    """mpcmp_warm_start_jerk_batch_device + mpcmp_solve_batch_device on the leg states (jmax None: the built-in initialiser)"""
    import torch
    L, dev = l0.shape[0], "cuda"
    t0, tf = torch.from_numpy(l0).to(dev), torch.from_numpy(lf).to(dev)
    mk = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)
    wx, wu, wT = mk(L, s2.N, s2.nx), mk(L, s2.N, s2.nu), mk(L)
    sx, su, sT = mk(L, s2.N, s2.nx), mk(L, s2.N, s2.nu), mk(L)
    inf = torch.zeros(L * M.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    warm = (0, 0, 0)
    if jmax is not None:
        s2.warm_start_jerk_device(L, t0.data_ptr(), tf.data_ptr(), jmax, wx.data_ptr(), wu.data_ptr(), wT.data_ptr())
        warm = (wx.data_ptr(), wu.data_ptr(), wT.data_ptr())
    s2.solve_device(L, t0.data_ptr(), tf.data_ptr(), sx.data_ptr(), su.data_ptr(), sT.data_ptr(), info=inf.data_ptr(), warm=warm)
    torch.cuda.synchronize()
    return sx.cpu().numpy(), su.cpu().numpy(), sT.cpu().numpy(), inf.cpu().numpy().view(M.INFO_DTYPE)


@pytest.fixture(scope="module")
def solved(M):
    """the route solves of the N = 7 context, shared by the solve, join and independence tests: {(nvia, with jmax): (inputs, outputs)}"""
    s = _solver(M, 2, 3)
    x0, xf = _states(1, 3)
    out = {}
    for nvia in MS:
        via = _vias(M, x0, xf, nvia, 1)
        for jm in (True, False):
            out[nvia, jm] = (via, s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M) if jm else None))
    return s, x0, xf, out


@pytest.mark.parametrize("nvia", MS)
@pytest.mark.parametrize("jm", [True, False], ids=["jerk_start", "builtin_start"])
def test_route_solve_is_the_plain_solve_of_its_legs_n7(M, solved, nvia, jm):
    s, x0, xf, out = solved
    via, r = out[nvia, jm]
    l0, lf, vq = s.route_legs(x0, via, xf, speed=0.5)
    assert same_bits(vq, r["via_qd"])
    L = l0.shape[0]
    s2 = _solver(M, 2, 3)
    sx, su, sT, info = _plain_legs_device(M, s2, l0, lf, _jmax(M) if jm else None)
    assert same_bits(r["sol_x"].reshape(sx.shape), sx) and same_bits(r["sol_u"].reshape(su.shape), su)
    assert same_bits(r["sol_T"].reshape(L), sT) and same_bits(r["info"].reshape(L), info)
    assert np.all(np.isfinite(sT)) and np.all(sT > 0)
    if nvia == 0:       # the one leg is (x0, xf) unchanged: mpcmp_solve_batch of the route's own states
        s3 = _solver(M, 2, 3)
        px, pu, pT, pi = s3.solve(x0, xf, s3.warm_start_jerk(x0, xf, _jmax(M)) if jm else None)
        assert same_bits(r["sol_x"][:, 0], px) and same_bits(r["sol_u"][:, 0], pu) and same_bits(r["sol_T"][:, 0], pT) and same_bits(r["info"][:, 0], pi)
        assert np.all(r["seam"]["state_jump_inf"] == 0) and np.all(r["seam"]["acc_jump_inf"] == 0)


@pytest.mark.parametrize("narm,sqp", [(1, 2), (2, 1)], ids=["n19_k_qp5", "dual_n19_k_qp3"])
def test_route_solve_is_the_plain_solve_of_its_legs_n19(M, narm, sqp):
    s, s2 = _solver(M, 6, sqp, narm, max_batch=6), _solver(M, 6, sqp, narm, max_batch=6)
    x0, xf = _states(narm, 3, off=20)
    via = _vias(M, x0, xf, 1, narm)
    r = s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M))
    l0, lf, _ = s.route_legs(x0, via, xf, speed=0.5)
    sx, su, sT, info = _plain_legs_device(M, s2, l0, lf, _jmax(M))
    assert same_bits(r["sol_x"].reshape(sx.shape), sx) and same_bits(r["sol_u"].reshape(su.shape), su)
    assert same_bits(r["sol_T"].reshape(-1), sT) and same_bits(r["info"].reshape(-1), info)
    assert np.all(np.isfinite(sT)) and np.all(sT > 0)
    rT, rinfo, seam, _ = join_np(M, r["sol_x"], r["sol_u"], r["sol_T"], r["info"])
    assert same_bits(r["route_T"], rT) and same_bits(r["route_info"], rinfo) and same_bits(r["seam"], seam)
    if narm == 2:
        with pytest.raises(M.MpcmpError):          # two arms need the jerk-limited start guess, as mpcmp_solve_batch does
            s.solve_route(x0, via, xf, speed=0.5)


def test_device_variant_matches_the_host_variant(M, solved):
    import torch
    s, x0, xf, out = solved
    nvia = 3
    via, r = out[nvia, True]
    B, L, dev = 3, 12, "cuda"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    mk = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=dev)
    rec = lambda n, dt: torch.zeros(n * dt.itemsize, dtype=torch.uint8, device=dev)
    t0, tv, tf, tsp = up(x0), up(via), up(xf), up(np.full(B, 0.5))
    sx, su, sT, rT, vo = mk(L, s.N, 14), mk(L, s.N, 7), mk(L), mk(B), mk(B, nvia, 7)
    inf, rinf, seam = rec(L, M.INFO_DTYPE), rec(B, M.INFO_DTYPE), rec(B, M.ROUTE_SEAM_DTYPE)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s.solve_route_device(B, nvia, t0.data_ptr(), tv.data_ptr(), tf.data_ptr(), sx.data_ptr(), su.data_ptr(), sT.data_ptr(), rT.data_ptr(),
                             rinf.data_ptr(), seam.data_ptr(), info=inf.data_ptr(), speed=tsp.data_ptr(), jmax=_jmax(M), via_qd_out=vo.data_ptr(),
                             stream=st.cuda_stream)
        smp = mk(B, 21, 29)
        s.sample_route_device(B, nvia, sx.data_ptr(), su.data_ptr(), sT.data_ptr(), 20, smp.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert same_bits(sx.cpu().numpy().reshape(r["sol_x"].shape), r["sol_x"]) and same_bits(sT.cpu().numpy().reshape(B, -1), r["sol_T"])
    assert same_bits(inf.cpu().numpy().view(M.INFO_DTYPE).reshape(B, -1), r["info"]) and same_bits(rT.cpu().numpy(), r["route_T"])
    assert same_bits(rinf.cpu().numpy().view(M.INFO_DTYPE), r["route_info"]) and same_bits(seam.cpu().numpy().view(M.ROUTE_SEAM_DTYPE), r["seam"])
    assert same_bits(vo.cpu().numpy(), r["via_qd"])
    assert same_bits(smp.cpu().numpy(), s.sample_route(r["sol_x"], r["sol_u"], r["sol_T"], 20))


# ---- 3. join ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvia", MS)
def test_join_matches_its_restatement(M, solved, nvia):
    s, x0, xf, out = solved
    via, r = out[nvia, True]
    rT, rinfo, seam, _ = join_np(M, r["sol_x"], r["sol_u"], r["sol_T"], r["info"])
    assert same_bits(r["route_T"], rT) and same_bits(r["route_info"], rinfo) and same_bits(r["seam"], seam)
    got = s.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"])
    assert same_bits(got[0], rT) and same_bits(got[1], rinfo) and same_bits(got[2], seam)
    if nvia:
        assert np.all(seam["acc_jump_inf"] > 0)          # accelerations are not continuous at a via, and the record says so
    # hand-made records: statuses, maxima with a NaN, ties of the longest leg, the first bad leg
    B, nl = 3, nvia + 1
    rng = np.random.default_rng(11)
    info = r["info"].copy(); sT = r["sol_T"].copy()
    info["status"] = rng.choice([0, 8, 16, 8 | 32, 2], size=(B, nl)); info["qp_capped"] = rng.integers(0, 3, (B, nl))
    info["last_alpha"] = rng.choice([1.0, 0.5, 0.25], size=(B, nl)); info["sqp_iters"] = rng.integers(1, 4, (B, nl))
    info["viol_l1"][0, -1] = np.nan
    sT[1, :] = 0.75                                        # every leg as long as the others: leg_longest = 0
    want = join_np(M, r["sol_x"], r["sol_u"], sT, info)
    got = s.route_join(r["sol_x"], r["sol_u"], sT, info)
    assert all(same_bits(g, w) for g, w in zip(got, want[:3]))
    assert got[2]["leg_longest"][1] == 0 and np.isnan(got[1]["viol_l1"][0])


def _clr(M, d, tm, tf, sp, ot, nh, st):
    return (d, tm, tf, sp, ot, nh, st)


def test_clearance_merge_matches_its_restatement(M, solved):
    s, x0, xf, out = solved
    via, r = out[3, True]
    free = _clr(M, 0.2, 0.3, -1.0, 4, 0, 0, 0)
    nopair = _clr(M, np.inf, -1.0, -1.0, -1, 0, 0, 0)
    clr = np.zeros((3, 4), dtype=M.CLEARANCE_DTYPE)
    # route 0: a tie of d_min between legs 1 and 2 (the lower leg wins), a hit only in legs 2 and 3
    rec = lambda rows: np.array(rows, dtype=M.CLEARANCE_DTYPE)
    clr[0] = rec([free, _clr(M, 0.05, 0.1, -1.0, 7, 1, 0, 0), _clr(M, 0.05, 0.2, 0.15, 9, -3, 2, M.CLR_HIT), _clr(M, 0.07, 0.4, 0.05, 2, 0, 1, M.CLR_HIT)])
    # route 1: a NaN leg among legs with hits
    clr[1] = rec([free, _clr(M, np.nan, -1.0, -1.0, -1, 0, 0, M.CLR_NAN), _clr(M, -0.01, 0.2, 0.1, 3, 0, 4, M.CLR_HIT), free])
    # route 2: no pair at all
    clr[2] = rec([nopair] * 4)
    want = join_np(M, r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr)
    got = s.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr)
    assert all(same_bits(g, w) for g, w in zip(got, want))
    c, T = got[3], r["sol_T"]
    assert c["sphere"][0] == 7 and c["other"][0] == 1 and c["t_min"][0] == 0.1 + T[0, 0]
    assert c["t_first"][0] == 0.15 + ((T[0, 0] + T[0, 1])) and c["n_hit"][0] == 3 and c["status"][0] == M.CLR_HIT
    assert np.isnan(c["d_min"][1]) and c["sphere"][1] == -1 and c["n_hit"][1] == 0 and c["status"][1] == M.CLR_NAN | M.CLR_HIT
    assert np.isinf(c["d_min"][2]) and c["t_min"][2] == -1 and c["sphere"][2] == -1 and c["status"][2] == 0


def test_candidates_are_checked_and_the_fastest_clear_one_is_kept(M):
    """plan K = 3 candidate routes per problem, check every leg, join, select: the pipeline of the issue, against the restated selection rule"""
    G, K, nvia = 2, 3, 1
    B, L = G * K, G * K * (nvia + 1)
    s = _solver(M, 2, 3, max_batch=L)
    a0, af = _states(1, G, off=40)
    x0, xf = np.repeat(a0, K, axis=0), np.repeat(af, K, axis=0)
    via = _vias(M, x0, xf, nvia, 1, seed=9, spread=0.6)
    via[::K] = 0.5 * (x0[::K, None, :7] + xf[::K, None, :7])          # candidate 0 of every group passes the midpoint of the direct move
    r = s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M))
    model = M.default_model()
    s.set_robot_spheres(M.link_spheres(model, 0.06, 0.08))
    obs = np.zeros((L, 1), dtype=M.OBSTACLE_DTYPE)                     # one sphere per problem, on the tool's path at the direct move's midpoint:
    for b in range(B):                                                 # obstacle sets are per batch slot = per leg slot, so every set M + 1 times
        p = M.tool_jacobian(model, 0.5 * (x0[b, :7] + xf[b, :7]))[1]
        for l in range(b * (nvia + 1), (b + 1) * (nvia + 1)):
            obs[l, 0] = M.obstacle(M.OBS_SPHERE, p, r=0.08)
    s.set_obstacles(obs)
    clr = s.clearance(r["sol_x"].reshape(L, s.N, 14), r["sol_T"].reshape(L), n_pts=50).reshape(B, nvia + 1)
    rT, rinfo, seam, rclr = s.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr)
    assert all(same_bits(g, w) for g, w in zip((rT, rinfo, seam, rclr), join_np(M, r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr)))
    assert np.all(rclr["status"][::K] != 0)                            # the candidate through the obstacle is seen
    group = np.repeat(np.arange(G), K).astype(np.int32)
    chosen = s.select_clear(rT, rinfo, rclr, group, G)
    assert np.array_equal(chosen, select_np(rT, rinfo, rclr, group, G))
    assert all(c == -1 or c % K != 0 for c in chosen)


# ---- 4. sampling -----------------------------------------------------------------------------------------------------------------------
LEG_T = {0: [[1.1], [0.77]], 1: [[0.9, 1.43], [1.21, 0.58]], 3: [[0.83, 1.27, 0.61, 1.09], [0.52, 0.91, 1.33, 0.47]]}


def _synthetic(nl, B, N, seed):
    r = np.random.default_rng(seed)
    k = np.linspace(0.0, 1.0, N)[None, None, :, None]
    ph = r.uniform(0, 2 * np.pi, (B, nl, 1, 14)); am = r.uniform(0.2, 0.8, (B, nl, 1, 14))
    sx = am * np.sin(2.0 * k + ph)
    su = r.uniform(0.5, 2.0, (B, nl, 1, 7)) * np.cos(3.0 * k + ph[..., :7])
    return np.ascontiguousarray(sx), np.ascontiguousarray(su)


@pytest.fixture(scope="module")
def sampler(M):
    return _solver(M, 2, 1)


@pytest.mark.parametrize("nvia", MS)
def test_route_samples_match_the_located_leg(M, sampler, nvia):
    s, n_pts, B = sampler, 50, 2
    sT = np.array(LEG_T[nvia])
    sx, su = _synthetic(nvia + 1, B, s.N, 21 + nvia)
    out = s.sample_route(sx, su, sT, n_pts)
    for b in range(B):
        R = 0.0; E = []
        for x in sT[b]:
            R += x; E.append(R)
        for i in range(n_pts + 1):
            t = i / n_pts * R
            assert all(abs(t - e) > 1e-9 * R for e in E[:-1]), (b, i)        # on the reference: no sample sits on a junction
            leg, tau = locate_np(list(sT[b]), t)
            if i == n_pts:
                leg, tau = nvia, 1.0
            ref = row_np(2, sx[b, leg], su[b, leg], tau)
            assert out[b, i, 0] == t and np.abs(out[b, i, 1:] - ref).max() < 1e-9, (b, i, leg, tau)


def test_junction_samples_are_the_later_legs_first_node(M, sampler):
    s = sampler
    sT = np.array([[1.0, 1.0, 2.0]])
    sx, su = _synthetic(3, 1, s.N, 33)
    out = s.sample_route(sx, su, sT, 8)
    assert np.array_equal(out[0, :, 0], np.arange(9) * 0.5)
    legs = s.sample(sx[0], su[0], sT[0], n_pts=1)                      # every leg at normalised times 0 and 1
    assert same_bits(out[0, 2, 1:], legs[1, 0, 1:]) and same_bits(out[0, 4, 1:], legs[2, 0, 1:]) and same_bits(out[0, 8, 1:], legs[2, 1, 1:])
    assert np.array_equal(out[0, 2, 1:15], sx[0, 1, 0]) and np.array_equal(out[0, 4, 1:15], sx[0, 2, 0]) and np.array_equal(out[0, 8, 1:15], sx[0, 2, -1])
    assert same_bits(out[0, 0, 1:], legs[0, 0, 1:])
    inner = s.sample(sx[0], su[0], sT[0], n_pts=2)                     # sample 1 (t = 0.5) is the middle of leg 0
    assert same_bits(out[0, 1, 1:], inner[0, 1, 1:])


def test_route_samples_read_the_payload_row_of_the_leg_slot(M, sampler):
    s, nvia, B = sampler, 1, 2
    sT = np.array(LEG_T[nvia])
    sx, su = _synthetic(nvia + 1, B, s.N, 22)
    empty = s.sample_route(sx, su, sT, 50)
    s.set_payloads(np.array([0.0, 3.0, 0.0, 0.0]))                     # leg slot 1 = the second leg of route 0 carries 3 kg
    try:
        heavy = s.sample_route(sx, su, sT, 50)
    finally:
        s.clear_payloads()
    in_leg1 = np.array([locate_np(list(sT[0]), i / 50 * (sT[0, 0] + sT[0, 1]))[0] == 1 for i in range(50)] + [True])
    assert np.array_equal(heavy[..., :22], empty[..., :22]) and np.array_equal(heavy[1], empty[1])
    assert np.array_equal(heavy[0, ~in_leg1], empty[0, ~in_leg1])
    assert np.abs(heavy[0, in_leg1, 22:] - empty[0, in_leg1, 22:]).max() > 0.5
    lumped = o.Model.from_buffer_copy(M.model_add_payload(M.default_model(), M.payload(3.0, M.default_model().tool[:])))
    i = int(np.nonzero(in_leg1)[0][3])
    leg, tau = locate_np(list(sT[0]), i / 50 * (sT[0, 0] + sT[0, 1]))
    assert np.abs(heavy[0, i, 1:] - row_np(2, sx[0, leg], su[0, leg], tau, lumped)).max() < 1e-9
    with pytest.raises(M.MpcmpError):                                  # fewer payload rows than leg slots
        s.set_payloads(np.zeros(3)); s.sample_route(sx, su, sT, 50)
    s.clear_payloads()


def test_a_nan_leg_time_gives_nan_rows_for_that_route_only(M, sampler):
    s = sampler
    sT = np.array(LEG_T[3])
    sx, su = _synthetic(4, 2, s.N, 24)
    good = s.sample_route(sx, su, sT, 50)
    sT[1, 2] = np.nan
    out = s.sample_route(sx, su, sT, 50)
    assert np.all(np.isnan(out[1])) and same_bits(out[0], good[0])


# ---- 5. independence and reproducibility -------------------------------------------------------------------------------------------------
def test_a_route_does_not_depend_on_its_batch(M, solved):
    s, x0, xf, out = solved
    via, r = out[3, True]
    again = s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M))
    assert all(same_bits(again[k], r[k]) for k in r)
    for b in (0, 2):
        alone = s.solve_route(x0[b:b + 1], via[b:b + 1], xf[b:b + 1], speed=0.5, jmax=_jmax(M))
        assert all(same_bits(alone[k], r[k][b:b + 1]) for k in r), b
        smp = s.sample_route(r["sol_x"], r["sol_u"], r["sol_T"], 20)
        assert same_bits(s.sample_route(alone["sol_x"], alone["sol_u"], alone["sol_T"], 20), smp[b:b + 1])


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def _raw_route(M, s, B, nvia, x0, via, xf, speed=None, null=None, L_out=None):
    """mpcmp_solve_route_batch into buffers preset to a sentinel: (rc, True if nothing was written)"""
    L = L_out or B * (nvia + 1)
    f = lambda *sh: np.full(sh, -7.0)
    bufs = dict(sx=f(L, s.N, s.nx), su=f(L, s.N, s.nu), sT=f(L), info=np.full(L * 8, -7.0), rT=f(B), rinfo=np.full(B * 8, -7.0), seam=np.full(B * 3, -7.0),
                vo=f(B, max(nvia, 1), s.nu))
    p = {k: (None if k == null else v.ctypes.data) for k, v in bufs.items()}
    jm = _jmax(M)
    rc = M.lib().mpcmp_solve_route_batch(s._ctx, B, nvia, None if null == "x0" else x0.ctypes.data, None if null == "via" else via.ctypes.data, None,
                                         None if speed is None else speed.ctypes.data, xf.ctypes.data, jm.ctypes.data, p["sx"], p["su"], p["sT"], p["info"],
                                         p["rT"], p["rinfo"], p["seam"], p["vo"])
    return rc, all(np.all(v == -7.0) for v in bufs.values())


def test_errors_return_einval_and_write_nothing(M):
    s = _solver(M, 2, 3, max_batch=8)
    x0, xf = _states(1, 3)
    via = _vias(M, x0, xf, 1, 1)
    ref = _solver(M, 2, 3, max_batch=8).solve(x0, xf)

    def usable():
        got = s.solve(x0, xf)
        assert all(same_bits(a, b) for a, b in zip(got, ref))

    big = _vias(M, x0, xf, 3, 1)
    assert _raw_route(M, s, 3, 3, x0, big, xf, L_out=12) == (-1, True); usable()             # L = 12 > max_batch = 8
    for null in ("x0", "via", "sx", "sT", "rT", "rinfo", "seam"):
        assert _raw_route(M, s, 3, 1, x0, via, xf, null=null) == (-1, True), null
    usable()
    for bad in (1.5, -0.1, np.nan):
        assert _raw_route(M, s, 3, 1, x0, via, xf, speed=np.array([0.5, bad, 1.0])) == (-1, True), bad
    with pytest.raises(M.MpcmpError):
        s.route_legs(x0, via, xf, speed=np.array([0.5, 2.0, 1.0]))
    xbad = x0.copy(); xbad[1, 3] = np.inf
    assert _raw_route(M, s, 3, 1, xbad, via, xf) == (-1, True)
    assert _raw_route(M, s, 0, 1, x0, via, xf, L_out=2)[0] == -1 and _raw_route(M, s, 3, -1, x0, via, xf, L_out=2)[0] == -1
    usable()
    # fewer rows than leg slots: every table
    s.set_bounds(s.bounds_table(n=4))
    assert _raw_route(M, s, 3, 1, x0, via, xf) == (-1, True)
    with pytest.raises(M.MpcmpError):
        s.route_legs(x0, via, xf)
    s.clear_bounds()
    s.set_time_windows(np.zeros(5), np.full(5, 10.0))
    assert _raw_route(M, s, 3, 1, x0, via, xf) == (-1, True)
    s.clear_time_windows()
    s.set_payloads(np.zeros(5))
    assert _raw_route(M, s, 3, 1, x0, via, xf) == (-1, True)
    s.clear_payloads()
    usable()
    assert _raw_route(M, s, 3, 1, x0, via, xf)[0] == 0                                       # the same call with everything in order
    usable()
    # the join and the sampler
    r = s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M))
    clr = np.zeros((3, 2), dtype=M.CLEARANCE_DTYPE); rc = np.zeros(3, dtype=M.CLEARANCE_DTYPE)
    d = lambda a: a.ctypes.data
    L_ = M.lib()
    assert L_.mpcmp_route_join(s._ctx, 3, 1, d(r["sol_x"]), d(r["sol_u"]), d(r["sol_T"]), d(r["info"]), d(clr), d(r["route_T"]), d(r["route_info"]),
                               d(r["seam"]), None) == -1
    assert L_.mpcmp_route_join(s._ctx, 3, 1, d(r["sol_x"]), d(r["sol_u"]), d(r["sol_T"]), None, None, d(r["route_T"]), d(r["route_info"]), d(r["seam"]), None) == -1
    assert L_.mpcmp_route_join(s._ctx, 5, 1, d(r["sol_x"]), d(r["sol_u"]), d(r["sol_T"]), d(r["info"]), d(clr), d(r["route_T"]), d(r["route_info"]),
                               d(r["seam"]), d(rc)) == -1
    out = np.full((3, 11, 29), -7.0)
    assert L_.mpcmp_sample_route_batch(s._ctx, 3, 1, d(r["sol_x"]), d(r["sol_u"]), d(r["sol_T"]), 0, d(out)) == -1
    assert L_.mpcmp_sample_route_batch(s._ctx, 3, 1, d(r["sol_x"]), None, d(r["sol_T"]), 10, d(out)) == -1
    assert L_.mpcmp_sample_route_batch(s._ctx, 5, 1, d(r["sol_x"]), d(r["sol_u"]), d(r["sol_T"]), 10, d(out)) == -1 and np.all(out == -7.0)
    usable()


def test_routes_are_refused_after_rh_init(M):
    s = _solver(M, 2, 3, max_batch=8)
    x0, xf = _states(1, 3)
    via = _vias(M, x0, xf, 1, 1)
    s.rh_init(x0, xf)
    assert _raw_route(M, s, 3, 1, x0, via, xf) == (-1, True)
    with pytest.raises(M.MpcmpError):
        s.route_legs(x0, via, xf)
    ref = _solver(M, 2, 3, max_batch=8).solve(x0, xf)
    assert all(same_bits(a, b) for a, b in zip(s.solve(x0, xf), ref))


# ---- 7. a context that plans routes plans single moves as before ----------------------------------------------------------------------------
def test_plain_solves_are_unchanged_by_a_route_solve(M):
    s = _solver(M, 2, 3)                                    # carry_multipliers off (the default): every solve starts from lambda = 0
    x0, xf = _states(1, 3)
    via = _vias(M, x0, xf, 3, 1)
    before = s.solve(x0, xf)
    s.solve_route(x0, via, xf, speed=0.5, jmax=_jmax(M))
    after = s.solve(x0, xf)
    assert all(same_bits(a, b) for a, b in zip(before, after))
    smp = s.sample(before[0], before[1], before[2], 20)
    one = s.sample_route(before[0][:, None], before[1][:, None], before[2][:, None], 20)      # M = 0: the plain sampler's rows, up to the rounding of
    assert np.abs(one - smp).max() < 1e-9                                                      # (i / n T) / T against i / n


def test_facade_plans_and_samples_routes(M):
    p = M.BatchMotionPlanner(max_batch=8, num_seg=2, sqp_iters=3)
    p.set_constraint_margins(*MARGINS)
    x0, xf = _states(1, 2)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    direct = p.solve_trajectory()
    t_direct = p.get_MPC_trajectory(20)[0]
    via = _vias(M, x0, xf, 2, 1)
    p.set_via_points(via)
    info = p.solve_trajectory()
    t, q, qd, qdd, tau = p.get_MPC_trajectory(20)
    sx, su, sT = p.solution()
    assert sT.shape == (2, 3) and info.shape == (2,) and q.shape == (2, 21, 7)
    assert np.array_equal(info["T"], sT[:, 0] + sT[:, 1] + sT[:, 2]) and np.array_equal(t[:, -1], info["T"])
    assert np.array_equal(q[:, 0], sx[:, 0, 0, :7]) and np.array_equal(q[:, -1], sx[:, -1, -1, :7])
    p.set_via_points(None)
    again = p.solve_trajectory()
    assert same_bits(again, direct) and same_bits(p.get_MPC_trajectory(20)[0], t_direct)
