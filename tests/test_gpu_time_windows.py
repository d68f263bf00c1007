"""Per-problem final-time windows, time scaling and time-synchronised solves on the GPU (mpcmp_set_time_windows*, mpcmp_time_scale_batch*,
mpcmp_solve_batch_synced*; include/mpcmp.h).  Covers: oracle parity per problem on every QP kernel path, with a problem's own row as its own
configuration; no change without rows (rows equal to the configuration's window, and a clear); the built-in initialiser under rows; the time
scaling against its NumPy restatement; the synchronised solve against the oracle chain; the error paths.  Run with -m gpu."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as o

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
T_OOB = 32                     # MPCMP_STATUS_T_OUT_OF_BOX
FAILED = 1 | 2 | 4 | 32        # the hard bits that take a problem out of its group

# kernel paths (a copy of test_gpu_solver_settings.PATHS): (id, num_seg, arms, environment at mpcmp_create, loop kernel of mpcmp_kernel_timing)
PATHS = [("k_qp1", 1, 1, {}, "k_qp"),
         ("k_qp2_2", 2, 1, {}, "k_qp2"), ("k_qp_2_v1", 2, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp2_4", 4, 1, {}, "k_qp2"), ("k_qp3_4", 4, 1, {"MPCMP_QP13": "3"}, "k_qp3"), ("k_qp_4_v1", 4, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp5_6", 6, 1, {}, "k_qp5"), ("k_qp3_6", 6, 1, {"MPCMP_QP19": "3"}, "k_qp3"),
         ("k_qp3_8", 8, 1, {}, "k_qp3"),
         ("k_qp3_6x2", 6, 2, {}, "k_qp3"), ("k_qp3_8x2", 8, 2, {}, "k_qp3")]
PATH = {p[0]: p for p in PATHS}
KINDS = ("default", "fixed", "window", "low_ub")      # the rows of the parity check, problem i takes KINDS[i % 4]
NPROB = 6
POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))      # (the oracle's solves release the GIL)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _limits():
    lim = o.default_limits()
    return MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]


def _states(narm, B, off):
    from mpc_motion_planner_amd import scenarios
    a0, af = scenarios.make_batch(B, MARGINS, stream_offset=off)
    if narm == 1:
        return a0, af
    b0, bf = scenarios.make_batch(B, MARGINS, stream_offset=off + 7919)
    return (np.stack([o.merge_arm_states([a0[b], b0[b]]) for b in range(B)]), np.stack([o.merge_arm_states([af[b], bf[b]]) for b in range(B)]))


def _osolve(narm, ocfg, x0, xf, wx, wu, wT):
    if narm == 1:
        return o.solve(ocfg, x0, xf, wx, wu, wT)
    return o.solve_multi(o.arm_models(o.DUAL_BASES), ocfg, x0, xf, wx, wu, wT)


def _omap(narm, cfgs, x0, xf, wx, wu, wT):
    """the oracle's solve of every problem b with its own configuration cfgs[b], in parallel"""
    return list(POOL.map(lambda b: _osolve(narm, cfgs[b], x0[b], xf[b], wx[b], wu[b], wT[b]), range(len(x0))))


def _ocfg(nseg, sqp, lbT=None, ubT=None):
    c = o.default_config(nseg, sqp, margins=MARGINS)
    if lbT is not None:
        c.lbT, c.ubT = lbT, ubT
    return c


def _check_solve(got, ref, what, idx=None):
    """the bar of test_gpu_solver_settings._check_solve: T <= 1e-6 relative, x <= 1e-6, u <= 1e-5, identical iteration counts, capped QPs, status
    words and last step lengths"""
    sx, su, sT, info = got
    for j, (xs, us, T, oi) in enumerate(ref):
        b = j if idx is None else idx[j]
        assert info["status"][b] == oi.status and info["qp_iters_total"][b] == oi.qp_iters_total and info["qp_capped"][b] == oi.qp_capped, \
            (what, b, info["status"][b], oi.status, info["qp_iters_total"][b], oi.qp_iters_total)
        assert info["last_alpha"][b] == oi.last_alpha, (what, b, info["last_alpha"][b], oi.last_alpha)
        assert abs(sT[b] - T) <= 1e-6 * abs(T), (what, b, sT[b], T)
        assert np.abs(sx[b] - xs).max() <= 1e-6, (what, b, np.abs(sx[b] - xs).max())
        assert np.abs(su[b] - us).max() <= 1e-5, (what, b, np.abs(su[b] - us).max())


def _same(a, b, what):
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True) if u.dtype.names is None else u.tobytes() == v.tobytes(), what


def time_scale_np(narm, x0, xf, sx, su, sT, T_new):
    """include/mpcmp.h, mpcmp_time_scale_batch, operation for operation"""
    s = sT / T_new
    ox = sx.copy()
    ox[:, 1:-1, 7 * narm:] = sx[:, 1:-1, 7 * narm:] * s[:, None, None]
    ox[:, 0] = x0
    ox[:, -1] = xf
    ou = su * (s * s)[:, None, None]
    return ox, ou, np.array(T_new, dtype=np.float64)


# ---- 1. oracle parity per problem on every kernel path -------------------------------------------------------------------------------------
_PROB = {}


def _parity_problems(narm, nseg):
    """(x0, xf, start guess, rows lbT / ubT, the oracle's answers with the rows and without) of the path's problems.  The rows are built from each
    problem's free optimum T* (an 8-iteration oracle solve): the default [0, 10], a fixed T = 1.3 T*, a window [1.2, 1.5] T*, and ubT = 0.7 T*"""
    key = (narm, nseg)
    if key not in _PROB:
        x0, xf = _states(narm, NPROB, 300 + 10 * nseg + narm)
        deep = _ocfg(nseg, 8)
        if narm == 1:
            warm = [o.warm_start(deep, x0[b], xf[b]) for b in range(NPROB)]
        else:
            warm = [o.warm_start_jerk_multi(nseg, *_limits(), x0[b], xf[b]) for b in range(NPROB)]
        wx, wu, wT = (np.array([w[i] for w in warm]) for i in range(3))
        Tstar = np.array([r[2] for r in _omap(narm, [deep] * NPROB, x0, xf, wx, wu, wT)])
        lb, ub = np.zeros(NPROB), np.full(NPROB, 10.0)
        for b in range(NPROB):
            k = KINDS[b % 4]
            if k == "fixed":
                lb[b] = ub[b] = 1.3 * Tstar[b]
            elif k == "window":
                lb[b], ub[b] = 1.2 * Tstar[b], 1.5 * Tstar[b]
            elif k == "low_ub":
                ub[b] = 0.7 * Tstar[b]
        ref = _omap(narm, [_ocfg(nseg, 3, lb[b], ub[b]) for b in range(NPROB)], x0, xf, wx, wu, wT)
        base = _omap(narm, [_ocfg(nseg, 3)] * NPROB, x0, xf, wx, wu, wT)
        _PROB[key] = (x0, xf, (wx, wu, wT), lb, ub, ref, base)
    return _PROB[key]


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_rows_vs_oracle_on_every_path(M, path):
    """3 SQP iterations per problem under its own row, against the oracle with that row as its configuration; the oracle first shows that every
    row other than the default changes its answer, and that a ubT below the optimum ends outside the box (status bit 32)"""
    _, nseg, narm, env, kname = PATH[path]
    x0, xf, warm, lb, ub, ref, base = _parity_problems(narm, nseg)
    for b in range(NPROB):
        k = KINDS[b % 4]
        r, q = ref[b], base[b]
        if k == "default":
            assert r[3].status == q[3].status and r[2] == q[2]
        else:
            assert abs(r[2] - q[2]) > 1e-6 * q[2], (path, b, k, "the row does not change the oracle's answer")
        if k == "low_ub":
            assert r[3].status & T_OOB, (path, b, r[3].status)
        if k == "fixed" and not r[3].status & T_OOB:
            assert abs(r[2] - lb[b]) <= 1e-9
    with _env(env):
        s = M.Solver(M.default_config(nseg, 3, margins=MARGINS), NPROB, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    assert s.kernel_timing()[0] == kname
    s.set_time_windows(lb, ub)
    got = s.solve(x0, xf, warm)
    _check_solve(got, ref, path)
    assert any(got[3]["status"][b] & T_OOB for b in range(NPROB))


# ---- 2. no change without rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,sqp", [(4, 20), (6, 2)], ids=["headline", "shipped"])
def test_config_rows_and_clear_change_nothing(M, nseg, sqp):
    """B = 1,024 from the jerk-limited start (bench.py): rows equal to [cfg.lbT, cfg.ubT] and a cleared context give the outputs of no rows, bit
    for bit; mixed rows in between do change them"""
    B = 1024
    cfg = M.default_config(nseg, sqp, margins=MARGINS)
    s = M.Solver(cfg, B)
    x0, xf = _states(1, B, 0)
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    plain = s.solve(x0, xf, warm)
    s.set_time_windows(np.full(B, cfg.lbT), np.full(B, cfg.ubT))
    _same(s.solve(x0, xf, warm), plain, "rows equal to the configuration's window")
    lb = np.where(np.arange(B) % 3 == 0, 1.2 * plain[2], 0.0)
    s.set_time_windows(lb, np.full(B, 10.0))
    mixed = s.solve(x0, xf, warm)
    assert not np.array_equal(mixed[2], plain[2])
    s.clear_time_windows()
    _same(s.solve(x0, xf, warm), plain, "after a clear")
    fresh = M.Solver(cfg, B)
    _same(fresh.solve(x0, xf, warm), plain, "a fresh context")


# ---- 3. the built-in initialiser -----------------------------------------------------------------------------------------------------------
def _quintic_np(nseg, x0, xf, T):
    """k_init's quintic at duration T, sampled at the collocation nodes (the end nodes are the given states)"""
    N = 3 * nseg + 1
    q0, v0, q1, v1 = x0[:7], x0[7:], xf[:7], xf[7:]
    h, T2 = q1 - q0, T * T
    T3 = T2 * T
    c = np.stack([q0, v0, np.zeros(7), (20.0 * h - (8.0 * v1 + 12.0 * v0) * T) / (2.0 * T3),
                  (-30.0 * h + (14.0 * v1 + 16.0 * v0) * T) / (2.0 * T3 * T), (12.0 * h - 6.0 * (v1 + v0) * T) / (2.0 * T3 * T2)], axis=1)
    ts = [-1.0, -0.5, 0.5, 1.0]
    x, u = np.zeros((N, 14)), np.zeros((N, 7))
    for k in range(N):
        sg = nseg - 1 if k == N - 1 else k // 3
        tt = (sg + 0.5 * (ts[k - 3 * sg] + 1.0)) / nseg * T
        x[k, :7] = c[:, 0] + tt * (c[:, 1] + tt * (c[:, 2] + tt * (c[:, 3] + tt * (c[:, 4] + tt * c[:, 5]))))
        x[k, 7:] = c[:, 1] + tt * (2 * c[:, 2] + tt * (3 * c[:, 3] + tt * (4 * c[:, 4] + tt * 5 * c[:, 5])))
        u[k] = 2 * c[:, 2] + tt * (6 * c[:, 3] + tt * (12 * c[:, 4] + tt * 20 * c[:, 5]))
    x[0], x[-1] = x0, xf
    return x, u


@pytest.mark.parametrize("nseg", [4, 6, 8])
def test_builtin_initialiser_under_rows(M, nseg):
    """rows whose lbT lies below the grid's duration give today's guess bit for bit; rows above it give the quintic at lbT; a ubT below it stops
    the grid at the first step past ubT"""
    B = 24
    s = M.Solver(M.default_config(nseg, 2, margins=MARGINS), B)
    x0, xf = _states(1, B, 500 + nseg)
    today = s.warm_start(x0, xf)
    T0 = today[2]
    kind = np.where(T0 < 5.0, np.arange(B) % 3, 0)          # (a grid that ran into cfg.ubT = 10 keeps its row's window at [0.5 T0, 10])
    assert (kind == 1).sum() >= 4 and (kind == 2).sum() >= 4
    lb = np.where(kind == 0, 0.5 * T0, np.where(kind == 1, 1.5 * T0, 0.0))
    ub = np.where(kind == 2, 0.5 * T0, 10.0)
    s.set_time_windows(lb, ub)
    wx, wu, wT = s.warm_start(x0, xf)
    for b in range(B):
        if kind[b] == 0:
            assert np.array_equal(wx[b], today[0][b]) and np.array_equal(wu[b], today[1][b]) and wT[b] == T0[b]
            continue
        if kind[b] == 1:
            T = lb[b]
        else:
            T = 0.05
            while not T * 1.05 > ub[b]:
                T *= 1.05
        assert wT[b] == T, (b, wT[b], T)
        x, u = _quintic_np(nseg, x0[b], xf[b], T)
        assert np.abs(wx[b] - x).max() <= 1e-14 * max(1.0, np.abs(x).max()), (b, np.abs(wx[b] - x).max())
        assert np.abs(wu[b] - u).max() <= 1e-14 * max(1.0, np.abs(u).max()), (b, np.abs(wu[b] - u).max())
    # the solve from the built-in start reads the same guess
    got = s.solve(x0, xf)
    ref = s.solve(x0, xf, (wx, wu, wT))
    _same(got, ref, "built-in start under rows")


# ---- 4. time scaling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 1), (6, 2), (8, 2)])
def test_time_scale_host_and_device_equal_numpy(M, nseg, narm):
    import torch
    B = 37
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    N, nx, nu = s.N, 14 * narm, 7 * narm
    rng = np.random.default_rng(nseg + narm)
    x0, xf = _states(narm, B, 40)
    sx, su = rng.uniform(-2, 2, (B, N, nx)), rng.uniform(-5, 5, (B, N, nu))
    sT, Tn = rng.uniform(0.5, 3, B), rng.uniform(0.5, 4, B)
    ref = time_scale_np(narm, x0, xf, sx, su, sT, Tn)
    _same(s.time_scale(x0, xf, sx, su, sT, Tn), ref, "host variant")
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x0, xf, sx, su, sT, Tn)]
    out = [torch.zeros_like(dev[2]), torch.zeros_like(dev[3]), torch.zeros_like(dev[4])]
    stream = torch.cuda.current_stream().cuda_stream
    s.time_scale_device(B, *[t.data_ptr() for t in dev], *[t.data_ptr() for t in out], stream=stream)
    torch.cuda.synchronize()
    _same([t.cpu().numpy() for t in out], ref, "device variant")
    # in place (the header allows it): ox = sx, ou = su, oT = sT; a problem's entries span several hundred to a thousand threads
    s.time_scale_device(B, *[t.data_ptr() for t in dev], dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    _same([t.cpu().numpy() for t in dev[2:5]], ref, "device variant in place")


# ---- 5. the synchronised solve -------------------------------------------------------------------------------------------------------------
def _oracle_pass2(narm, nseg, sqp, x0, xf, gx, gu, gT, idx):
    """the oracle's pass 2 of the problems idx: from the given (stretched) guesses, window [gT, gT]"""
    cfgs = {b: _ocfg(nseg, sqp, gT[b], gT[b]) for b in idx}
    return list(POOL.map(lambda b: _osolve(narm, cfgs[b], x0[b], xf[b], gx[b], gu[b], gT[b]), idx))


def _synced_check(M, s, narm, nseg, sqp, x0, xf, warm, group, n_groups, ub=None):
    """one synchronised solve checked against the plain solve, the NumPy group maximum, the NumPy stretch and the oracle's pass 2; returns
    (group_T, re-solved indices).  Pass 1 is checked against the oracle at the bar of _check_solve.  Pass 2 of the oracle starts from the NumPy
    stretch of the GPU's pass-1 solution to the GPU's group time, not from the oracle's own pass 1: the group time is the GPU's T bit for bit, and
    start guesses 1e-7 apart may move an ADMM termination test by a period and change the iteration count that must match exactly.  The stretch
    itself is the header's arithmetic (checked against the kernel bit for bit, and against the collocation defects in test_time_windows_host)"""
    import torch
    B = x0.shape[0]
    plain = s.solve(x0, xf, warm)
    sx, su, sT, info, gT = s.solve_synced(x0, xf, group, warm, n_groups=n_groups)
    assert gT.shape == (n_groups,)
    # pass 1 is the plain solve: the oracle agrees with it
    cfgs = [_ocfg(nseg, sqp) if ub is None else _ocfg(nseg, sqp, 0.0, ub[b]) for b in range(B)]       # (ub: the rows in force)
    _check_solve(plain, _omap(narm, cfgs, x0, xf, *warm), ("pass 1", nseg, narm))
    # group times: the NumPy maximum over the eligible members of the plain solve's T, bit for bit
    elig = (group >= 0) & (group < n_groups) & ((plain[3]["status"] & FAILED) == 0)
    want = np.array([plain[2][elig & (group == g)].max() if (elig & (group == g)).any() else np.nan for g in range(n_groups)])
    assert np.array_equal(gT, want, equal_nan=True), (gT, want)
    Tg = np.full(B, np.nan)
    Tg[elig] = want[group[elig]]
    re = elig & (plain[2] < Tg)
    idx = np.nonzero(re)[0]
    keep = np.nonzero(~re)[0]
    # every problem not re-solved: its plain outputs, bit for bit
    for a, p in zip((sx, su, sT), plain[:3]):
        assert np.array_equal(a[keep], p[keep])
    assert info[keep].tobytes() == plain[3][keep].tobytes()
    # the re-solved: the oracle's pass 2 from the NumPy stretch of the pass-1 solution to the group time
    if len(idx):
        Tn = np.where(re, Tg, plain[2])
        g = time_scale_np(narm, x0, xf, plain[0], plain[1], plain[2], Tn)
        ref = _oracle_pass2(narm, nseg, sqp, x0, xf, g[0], g[1], g[2], list(idx))
        _check_solve((sx, su, sT, info), ref, ("pass 2", nseg, narm), idx=list(idx))
        for b in idx:
            if not info["status"][b] & T_OOB:
                assert abs(sT[b] - Tg[b]) <= 1e-9, (b, sT[b], Tg[b])
    # the device variant: the same outputs, bit for bit
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x0, xf) + tuple(warm)]
    dg = torch.from_numpy(np.ascontiguousarray(group.astype(np.int32))).cuda()
    ox, ou, oT = torch.zeros_like(dev[2]), torch.zeros_like(dev[3]), torch.zeros_like(dev[4])
    oi = torch.zeros(B * 64, dtype=torch.uint8, device="cuda")
    og = torch.zeros(max(n_groups, 1), dtype=torch.float64, device="cuda")
    s.solve_synced_device(B, dev[0].data_ptr(), dev[1].data_ptr(), dg.data_ptr(), n_groups, ox.data_ptr(), ou.data_ptr(), oT.data_ptr(),
                          oi.data_ptr(), og.data_ptr(), warm=(dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr()),
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same([ox.cpu().numpy(), ou.cpu().numpy(), oT.cpu().numpy(), og.cpu().numpy()[:n_groups]], [sx, su, sT, gT], "device variant")
    assert oi.cpu().numpy().tobytes() == info.tobytes()
    return gT, idx


@pytest.mark.parametrize("nseg,sqp", [(4, 6), (6, 2)], ids=["n13", "n19"])
def test_synced_solve_vs_oracle_chain(M, nseg, sqp):
    """B = 64: eight groups of about seven plus ungrouped problems; then the same with an empty group and a group whose members all end outside
    their windows (no eligible member: NaN, nobody of it re-solved)"""
    B = 64
    s = M.Solver(M.default_config(nseg, sqp, margins=MARGINS), B)
    x0, xf = _states(1, B, 700 + nseg)
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    group = (np.arange(B) % 9 - 1).astype(np.int32)          # -1 = ungrouped, 0 .. 7
    gT, idx = _synced_check(M, s, 1, nseg, sqp, x0, xf, warm, group, 8)
    assert np.isfinite(gT).all() and len(idx) >= 8
    # group 7's members all get a ubT far below their time (status bit 32: not eligible); group 8 has no member
    plain = s.solve(x0, xf, warm)
    ub = np.where(group == 7, 0.3 * plain[2], 10.0)
    s.set_time_windows(np.zeros(B), ub)
    assert all(s.solve(x0, xf, warm)[3]["status"][group == 7] & T_OOB)
    gT, idx = _synced_check(M, s, 1, nseg, sqp, x0, xf, warm, group, 9, ub=ub)
    assert np.isnan(gT[7]) and np.isnan(gT[8]) and np.isfinite(gT[:7]).all()
    assert not (group[idx] == 7).any()
    s.clear_time_windows()


def test_synced_solve_dual_arm(M):
    """two arms, N = 25, B = 4: three problems in one group, one on its own"""
    nseg, sqp, B = 8, 1, 4
    s = M.Solver(M.default_config(nseg, sqp, margins=MARGINS), B, models=M.arm_models(M.DUAL_BASES))
    x0, xf = _states(2, B, 900)
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    group = np.array([0, 0, -1, 0], dtype=np.int32)
    gT, idx = _synced_check(M, s, 2, nseg, sqp, x0, xf, warm, group, 1)
    assert np.isfinite(gT[0]) and len(idx) >= 1


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors(M):
    B = 8
    cfg = M.default_config(4, 2, margins=MARGINS)
    s = M.Solver(cfg, B)
    x0, xf = _states(1, B, 60)
    plain = s.solve(x0, xf)

    def einval(fn, *a, **k):
        with pytest.raises(M.MpcmpError) as e:
            fn(*a, **k)
        assert e.value.code == -1, str(e.value)
        return str(e.value)

    # more problems than rows: nothing is written, the rows stay
    s.set_time_windows(np.zeros(B - 1), np.full(B - 1, 10.0))
    assert "final-time rows" in einval(s.solve, x0, xf)
    einval(s.warm_start, x0, xf)
    einval(s.qp, x0, xf, plain[0], plain[1], plain[2])
    einval(s.solve_synced, x0, xf, np.zeros(B))
    _same(s.solve(x0[:B - 1], xf[:B - 1]), [a[:B - 1] for a in plain], "rows of the solve as before")
    # bad rows: each kind; nothing changes (the B - 1 rows above stay in force)
    for lb, ub in ((np.nan, 1.0), (1.0, np.nan), (2.0, 1.0), (np.inf, np.inf), (-np.inf, -np.inf), (-0.1, 1.0)):
        L, U = np.zeros(B), np.full(B, 10.0)
        L[3], U[3] = lb, ub
        assert "row 3" in einval(s.set_time_windows, L, U)
        einval(s.solve, x0, xf)
    einval(s.set_time_windows, np.zeros(B + 1), np.full(B + 1, 10.0))      # more rows than the context holds
    s.clear_time_windows()
    _same(s.solve(x0, xf), plain, "after the rejections and a clear")
    # a group id out of range (host variant), warm_* given in part
    g = np.zeros(B, dtype=np.int32); g[5] = -2
    assert "group[5]" in einval(s.solve_synced, x0, xf, g)
    import ctypes as C
    p = plain[0].ctypes.data_as(C.c_void_p)
    gg = np.zeros(B, dtype=np.int32)
    assert M.lib().mpcmp_solve_batch_synced(s._ctx, B, x0.ctypes.data_as(C.c_void_p), xf.ctypes.data_as(C.c_void_p), p, None, None,
                                            gg.ctypes.data_as(C.c_void_p), 1, p, p, p, None, None) == -1
    gg[0] = 1
    assert M.lib().mpcmp_solve_batch_synced(s._ctx, B, x0.ctypes.data_as(C.c_void_p), xf.ctypes.data_as(C.c_void_p), None, None, None,
                                            gg.ctypes.data_as(C.c_void_p), 1, p, p, p, None, None) == -1
    # the receding-horizon driver: rows set -> mpcmp_rh_init refuses; a loop running -> the setters refuse
    s.set_time_windows(np.zeros(B), np.full(B, 10.0))
    assert "receding-horizon" in einval(s.rh_init, x0, xf)
    s.clear_time_windows()
    s.rh_init(x0, xf)
    assert "receding-horizon" in einval(s.set_time_windows, np.zeros(B), np.full(B, 10.0))
    einval(s.set_time_windows_device, B, 1, 1, 0)


def test_synced_solve_leaves_the_next_solve_as_a_plain_one(M):
    """N = 25, two arms, carried multipliers: the skipped problems' QP kernels run in pass 2 (k_qp3 has no retirement exit there) and may add to their
    status words; those are put back, so the next solve of a problem that was not re-solved equals the one after a plain solve, bit for bit"""
    nseg, B = 8, 4
    cfg = M.default_config(nseg, 1, margins=MARGINS, carry_multipliers=1)
    s = M.Solver(cfg, B, models=M.arm_models(M.DUAL_BASES))
    t = M.Solver(cfg, B, models=M.arm_models(M.DUAL_BASES))
    x0, xf = _states(2, B, 930)
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    group = np.array([0, 0, -1, 0], dtype=np.int32)
    synced = s.solve_synced(x0, xf, group, warm, n_groups=1)
    plain = t.solve(x0, xf, warm)
    keep = [b for b in range(B) if synced[2][b] == plain[2][b] and synced[3][b].tobytes() == plain[3][b].tobytes()]
    assert 2 in keep and len(keep) < B              # (the ungrouped one and the group's slowest are not re-solved; the others are)
    a, b = s.solve(x0, xf, warm), t.solve(x0, xf, warm)
    for i in keep:
        for u, v in zip(a[:3], b[:3]):
            assert np.array_equal(u[i], v[i]), i
        assert a[3][i].tobytes() == b[3][i].tobytes(), i


def test_planner_final_time_window(M):
    """BatchMotionPlanner.set_final_time_window: scalars apply to every problem, and the next solve_trajectory equals Solver.solve under those rows
    from the same jerk-limited start, bit for bit; lbT == ubT pulls every final time toward that duration; None clears at once, and the next
    solve equals a planner that never had a window"""
    from mpc_motion_planner_amd import scenarios
    B = 8
    x0, xf = scenarios.make_batch(B, MARGINS, stream_offset=950)

    def planner():
        p = M.BatchMotionPlanner(max_batch=B, num_seg=4, sqp_iters=6)
        p.set_constraint_margins(*MARGINS)
        p.set_current_state(x0[:, :7], x0[:, 7:])
        p.set_target_state(xf[:, :7], xf[:, 7:])
        return p

    p, ref = planner(), planner()
    ref.solve_trajectory()
    T_free = ref.solution()[2]
    s = M.Solver(p.cfg, B)
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    for lb, ub in ((2.4, None), (1.5 * T_free, 2.0 * T_free)):
        p.set_final_time_window(lb, ub)
        info = p.solve_trajectory()
        assert p._solver.time_window_rows == B
        s.set_time_windows(np.broadcast_to(lb, (B,)), np.broadcast_to(lb if ub is None else ub, (B,)))
        _same(list(p.solution()) + [info], list(s.solve(x0, xf, warm)), ("planner vs Solver", lb))
    p.set_final_time_window(2.4)
    p.solve_trajectory()
    assert np.abs(p.solution()[2] - 2.4).mean() < np.abs(T_free - 2.4).mean()
    p.set_final_time_window(None)
    assert p._solver.time_window_rows == 0
    info = p.solve_trajectory()
    _same(list(p.solution()) + [info], list(ref.solution()) + [ref.info], "after the window is removed")
