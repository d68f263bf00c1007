"""Per-problem bounds on the GPU (mpcmp_set_bounds[_device], include/mpcmp.h): row i = the six bound tables of problem i.  Covers: oracle parity
per problem on every QP kernel path, with a problem's own row copied into its own oracle configuration; no change without rows (rows equal to the
configuration, and a clear); the built-in initialiser and mpcmp_qp_batch under rows; batch-order independence; the synchronised solve; rows
together with payload and final-time rows; the device setter; pose targets under rows; the error paths.  Run with -m gpu.

What is NOT asserted, on purpose: that a returned iterate respects its row to tolerance.  ADMM is truncated at qp_iters, most QPs are capped, and an
iterate may exceed a row slightly (interior |qd| up to 1.03 - 1.07 of the slow row's bound on 1 - 2 of 20 problems in the oracle): parity with the
oracle and the status word are the properties checked."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as o

pytestmark = pytest.mark.gpu

CTX_MARGINS = (0.9, 0.9, 0.5, 0.9)              # the configuration of every context (mpcmp_set_margins sets the height 0.05)
STATE_MARGINS = (0.9, 0.4, 0.5, 0.9, 0.1)       # velocity margin 0.4: every start and target velocity lies inside every row, the slow one included
JERK_MARGIN = 0.1
HARD = 1 | 2 | 4 | 32                           # NAN | NOT_PD | XCH_DEAD | T_OUT_OF_BOX
TABLES = ("lbx", "ubx", "lbu", "ubu", "lbg", "ubg")

# kernel paths (a copy of test_gpu_time_windows.PATHS): (id, num_seg, arms, environment at mpcmp_create, loop kernel of mpcmp_kernel_timing)
PATHS = [("k_qp1", 1, 1, {}, "k_qp"),
         ("k_qp2_2", 2, 1, {}, "k_qp2"), ("k_qp_2_v1", 2, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp2_4", 4, 1, {}, "k_qp2"), ("k_qp3_4", 4, 1, {"MPCMP_QP13": "3"}, "k_qp3"), ("k_qp_4_v1", 4, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp5_6", 6, 1, {}, "k_qp5"), ("k_qp3_6", 6, 1, {"MPCMP_QP19": "3"}, "k_qp3"),
         ("k_qp3_8", 8, 1, {}, "k_qp3"),
         ("k_qp3_6x2", 6, 2, {}, "k_qp3"), ("k_qp3_8x2", 8, 2, {}, "k_qp3")]
PATH = {p[0]: p for p in PATHS}
KINDS = ("default", "slow", "weak", "narrow", "floor", "locked")       # problem i takes KINDS[i % 6]
NPROB = 12
SQP = {1: 3, 2: 3, 4: 3, 6: 2, 8: 2}            # SQP iterations of the parity check per num_seg
# states of a path: scenarios.make_batch(..., stream_offset = 900 + num_seg), the second arm 7919 further on (none had to be moved: the oracle alone
# meets the conditions of the parity check on every (num_seg, arms) below)
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


def _solver(M, path, B, sqp=None, **kw):
    _, nseg, narm, env, kname = PATH[path]
    with _env(env):
        s = M.Solver(M.default_config(nseg, SQP[nseg] if sqp is None else sqp, margins=CTX_MARGINS, **kw), B,
                     models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)
    assert s.kernel_timing()[0] == kname
    return s


def _row(M, kind):
    """the row of a kind, before the problem-dependent entries of `locked`"""
    if kind == "slow":
        return M.bounds_from_margins(0.9, 0.45, 0.25, 0.9, 0.05)
    if kind == "weak":
        return M.bounds_from_margins(0.9, 0.9, 0.5, 0.5, 0.05)
    if kind == "narrow":
        return M.bounds_from_margins(0.8, 0.9, 0.5, 0.9, 0.05)
    r = M.bounds_from_margins(0.9, 0.9, 0.5, 0.9, 0.05)
    if kind == "floor":
        r["lbg"][7] = 0.25
    return r


def _problems(M, narm, B, off, kinds=KINDS):
    """states and rows of B problems, problem i of kind kinds[i % len(kinds)].  A locked problem starts at its target's joint-6 angle with both
    joint-6 velocities zero, and its row pins that joint there (two arms: the row applies to both, so both arms share the angle of arm 0)"""
    from mpc_motion_planner_amd import scenarios
    a0, af = scenarios.make_batch(B, STATE_MARGINS, stream_offset=off)
    if narm == 2:
        b0, bf = scenarios.make_batch(B, STATE_MARGINS, stream_offset=off + 7919)
    rows = np.zeros(B, dtype=M.BOUNDS_DTYPE)
    for i in range(B):
        k = kinds[i % len(kinds)]
        rows[i] = _row(M, k)
        if k == "locked":
            q6 = af[i, 6]
            for x in (a0, af) + ((b0, bf) if narm == 2 else ()):
                x[i, 6], x[i, 13] = q6, 0.0
            rows["lbx"][i, 6] = rows["ubx"][i, 6] = q6
            rows["lbx"][i, 13] = rows["ubx"][i, 13] = 0.0
    if narm == 1:
        return a0, af, rows
    return (np.stack([o.merge_arm_states([a0[b], b0[b]]) for b in range(B)]), np.stack([o.merge_arm_states([af[b], bf[b]]) for b in range(B)]), rows)


def _ocfg(nseg, sqp, row=None, **kw):
    """the oracle's configuration of the contexts here, with a problem's row copied into its six tables"""
    c = o.default_config(nseg, sqp, margins=CTX_MARGINS, **kw)
    if row is not None:
        for name in TABLES:
            for i, v in enumerate(row[name]):
                getattr(c, name)[i] = v
    return c


def _owarm(narm, ocfg, x0, xf):
    """the oracle's start guess of one problem under its own row: the built-in initialiser, or (two arms) the jerk-limited one with the row's
    velocity and acceleration limits"""
    if narm == 1:
        return o.warm_start(ocfg, x0, xf)
    return o.warm_start_jerk_multi(ocfg.num_seg, np.array(ocfg.ubx[7:14]), np.array(ocfg.ubu[:]), JERK_MARGIN * o.default_limits()["jmax"], x0, xf)


def _osolve(narm, ocfg, x0, xf, wx, wu, wT, model=None):
    if narm == 1:
        return o.solve(ocfg, x0, xf, wx, wu, wT, model=model)
    return o.solve_multi(o.arm_models(o.DUAL_BASES), ocfg, x0, xf, wx, wu, wT)


def _omap(narm, cfgs, x0, xf, wx, wu, wT):
    return list(POOL.map(lambda b: _osolve(narm, cfgs[b], x0[b], xf[b], wx[b], wu[b], wT[b]), range(len(x0))))


def _check_solve(got, ref, what, idx=None):
    """the bar of test_gpu_solver_settings / test_gpu_time_windows: identical status word, iteration count, capped QPs and last step length;
    T <= 1e-6 relative, x <= 1e-6, u <= 1e-5"""
    sx, su, sT, info = got
    for j, (xs, us, T, oi) in enumerate(ref):
        b = j if idx is None else idx[j]
        print("%s problem %d: status %d / %d, qp_iters %d / %d, capped %d / %d, alpha %g / %g, dT %.3g, dx %.3g, du %.3g"
              % (what, b, info["status"][b], oi.status, info["qp_iters_total"][b], oi.qp_iters_total, info["qp_capped"][b], oi.qp_capped,
                 info["last_alpha"][b], oi.last_alpha, abs(sT[b] - T), np.abs(sx[b] - xs).max(), np.abs(su[b] - us).max()))
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
        assert np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes(), what


# ---- 1. oracle parity per problem on every kernel path -------------------------------------------------------------------------------------
_PROB = {}


def _parity_problems(M, narm, nseg):
    """(x0, xf, rows, start guess, the oracle's answers under the rows and under the default row) of a (num_seg, arms) pair"""
    key = (narm, nseg)
    if key not in _PROB:
        sqp = SQP[nseg]
        x0, xf, rows = _problems(M, narm, NPROB, 900 + nseg)
        cfgs = [_ocfg(nseg, sqp, rows[b]) for b in range(NPROB)]
        warm = list(POOL.map(lambda b: _owarm(narm, cfgs[b], x0[b], xf[b]), range(NPROB)))
        wx, wu, wT = (np.array([w[i] for w in warm]) for i in range(3))
        ref = _omap(narm, cfgs, x0, xf, wx, wu, wT)
        base = _omap(narm, [_ocfg(nseg, sqp)] * NPROB, x0, xf, wx, wu, wT)
        _PROB[key] = (x0, xf, rows, (wx, wu, wT), ref, base)
    return _PROB[key]


def _oracle_conditions(path, ref, base):
    """asserted on the oracle's answers alone, so that the check cannot pass by comparing two failures or two copies of the default: no hard bit,
    and at least half of the ten non-default problems differ from the oracle's answer to the same problem under the default row by > 1e-3 in x"""
    for b in range(NPROB):
        assert ref[b][3].status & HARD == 0, (path, b, KINDS[b % 6], ref[b][3].status)
    other = [b for b in range(NPROB) if KINDS[b % 6] != "default"]
    moved = [b for b in other if np.abs(ref[b][0] - base[b][0]).max() > 1e-3]
    print("%s: %d of %d non-default problems differ from the default row's answer by > 1e-3 (%s)" % (path, len(moved), len(other), moved))
    assert 2 * len(moved) >= len(other), (path, moved)
    for b in range(NPROB):
        if KINDS[b % 6] == "default":
            assert np.array_equal(ref[b][0], base[b][0]) and ref[b][2] == base[b][2]


@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_rows_vs_oracle_on_every_path(M, path):
    """12 problems of six kinds in ONE mpcmp_solve_batch with the rows set, against the oracle called per problem with the row in its config"""
    _, nseg, narm, env, kname = PATH[path]
    x0, xf, rows, warm, ref, base = _parity_problems(M, narm, nseg)
    _oracle_conditions(path, ref, base)
    s = _solver(M, path, NPROB)
    s.set_bounds(rows)
    _check_solve(s.solve(x0, xf, warm), ref, path)


# ---- 2. no change without rows, or with neutral rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [p[0] for p in PATHS])
def test_config_rows_and_clear_change_nothing(M, path):
    """rows equal to mpcmp_bounds_from_config(cfg) give the outputs of the same context before any setter call, bit for bit; so does a clear after
    mixed rows (which do change them); and mpcmp_warm_start_batch the same (one arm)"""
    _, nseg, narm, env, kname = PATH[path]
    x0, xf, rows, warm, ref, base = _parity_problems(M, narm, nseg)
    s = _solver(M, path, NPROB)
    plain = s.solve(x0, xf, warm)
    init = s.warm_start(x0, xf) if narm == 1 else None
    neutral = s.bounds_table(n=NPROB)
    assert all(neutral[b].tobytes() == M.bounds_from_config(s.cfg).tobytes() for b in range(NPROB))
    s.set_bounds(neutral)
    _same(s.solve(x0, xf, warm), plain, (path, "rows equal to the configuration"))
    if narm == 1:
        _same(s.warm_start(x0, xf), init, (path, "initialiser, rows equal to the configuration"))
    s.set_bounds(rows)
    mixed = s.solve(x0, xf, warm)
    assert not np.array_equal(mixed[0], plain[0])
    s.clear_bounds()
    _same(s.solve(x0, xf, warm), plain, (path, "after a clear"))
    if narm == 1:
        _same(s.warm_start(x0, xf), init, (path, "initialiser after a clear"))


@pytest.mark.parametrize("nseg,sqp", [(4, 20), (6, 2)], ids=["headline", "shipped"])
def test_config_rows_change_nothing_at_1024(M, nseg, sqp):
    """B = 1,024 from the jerk-limited start (the benchmark's batch, split over streams: a part's rows start at its b0)"""
    B = 1024
    from mpc_motion_planner_amd import scenarios
    margins = (0.9, 0.9, 0.5, 0.9, 0.1)
    cfg = M.default_config(nseg, sqp, margins=margins)
    s = M.Solver(cfg, B)
    x0, xf = scenarios.make_batch(B, margins)
    warm = s.warm_start_jerk(x0, xf, margins[4] * M.default_limits()["jmax"])
    plain = s.solve(x0, xf, warm)
    s.set_bounds(s.bounds_table(n=B))
    _same(s.solve(x0, xf, warm), plain, "rows equal to the configuration")
    # one row differs, in the last part of the split: that problem alone changes
    t = s.bounds_table(n=B)
    t[B - 3] = M.bounds_from_margins(0.9, 0.45, 0.25, 0.9, 0.05)
    s.set_bounds(t)
    one = s.solve(x0, xf, warm)
    diff = [b for b in range(B) if not np.array_equal(one[0][b], plain[0][b])]
    assert diff == [B - 3], diff
    s.clear_bounds()
    _same(s.solve(x0, xf, warm), plain, "after a clear")


# ---- 3. the built-in initialiser and mpcmp_qp_batch under rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [4, 6, 8])
def test_builtin_initialiser_under_rows(M, nseg):
    """mpcmp_warm_start_batch against the oracle's warm_start under each problem's row (the feasibility test is what reads the row: the slow row's
    guess is about twice as long as the default's), and the solve with warm_* NULL starts from that guess"""
    B = 24
    x0, xf, rows = _problems(M, 1, B, 500 + nseg)
    s = M.Solver(M.default_config(nseg, 2, margins=CTX_MARGINS), B)
    T_cfg = s.warm_start(x0, xf)[2]
    s.set_bounds(rows)
    wx, wu, wT = s.warm_start(x0, xf)
    for b in range(B):
        xg, ug, T = o.warm_start(_ocfg(nseg, 2, rows[b]), x0[b], xf[b])
        assert abs(wT[b] - T) <= 1e-12 * T, (b, wT[b], T)
        assert np.abs(wx[b] - xg).max() <= 1e-9 and np.abs(wu[b] - ug).max() <= 1e-9 * max(1.0, np.abs(ug).max()), (b, np.abs(wx[b] - xg).max())
    slow = np.arange(B) % 6 == 1
    print("initialiser, N = %d: T(slow row) / T(config) = %s" % (3 * nseg + 1, np.round(wT[slow] / T_cfg[slow], 3)))
    # (half the speed: twice the time; half the acceleration: 1.41 times; less where the grid runs into ubT)
    assert (wT[slow] >= T_cfg[slow]).all() and 2 * (wT[slow] > 1.3 * T_cfg[slow]).sum() >= slow.sum()
    assert np.array_equal(wT[np.arange(B) % 6 == 0], T_cfg[np.arange(B) % 6 == 0])
    _same(s.solve(x0, xf), s.solve(x0, xf, (wx, wu, wT)), "built-in start under rows")


@pytest.mark.parametrize("path", ["k_qp2_4", "k_qp3_6"])
def test_qp_batch_under_rows(M, path):
    """one QP at the start guess under each problem's row against the oracle's debug_qp (the bar of test_gpu_solver_settings._check_qp)"""
    _, nseg, narm, env, kname = PATH[path]
    x0, xf, rows, warm, ref, base = _parity_problems(M, narm, nseg)
    s = _solver(M, path, NPROB)
    p0, y0, it0 = s.qp(x0, xf, *warm)
    s.set_bounds(rows)
    p, y, it = s.qp(x0, xf, *warm)
    changed = 0
    for b in range(NPROB):
        pr, yr, itr = o.debug_qp(_ocfg(nseg, 1, rows[b]), x0[b], xf[b], warm[0][b], warm[1][b], warm[2][b])
        assert it[b] == itr, (path, b, it[b], itr)
        assert np.abs(p[b] - pr).max() <= 1e-7 * (1 + np.abs(pr).max()), (path, b, np.abs(p[b] - pr).max())
        assert np.abs(y[b] - yr).max() <= 1e-6 * (1 + np.abs(yr).max()), (path, b, np.abs(y[b] - yr).max())
        changed += b % 6 != 0 and not np.array_equal(p[b], p0[b])
        if b % 6 == 0:
            assert np.array_equal(p[b], p0[b]) and it[b] == it0[b]
    assert changed >= 5, changed


# ---- 4. batch-order independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["k_qp2_4", "k_qp5_6", "k_qp3_8x2"])
def test_outputs_do_not_depend_on_the_position_in_the_batch(M, path):
    """a problem with its row: the same outputs wherever it stands in the batch and whatever rows stand around it, bit for bit"""
    _, nseg, narm, env, kname = PATH[path]
    x0, xf, rows, warm, ref, base = _parity_problems(M, narm, nseg)
    s = _solver(M, path, NPROB)
    s.set_bounds(rows)
    a = s.solve(x0, xf, warm)
    perm = np.random.default_rng(3).permutation(NPROB)
    s.set_bounds(rows[perm])
    b = s.solve(x0[perm], xf[perm], tuple(w[perm] for w in warm))
    _same(b, [u[perm] for u in a], (path, "permuted"))
    # alone, in slot 0, for three of them
    for i in (1, 5, 10):
        s.set_bounds(rows[i:i + 1])
        c = s.solve(x0[i:i + 1], xf[i:i + 1], tuple(w[i:i + 1] for w in warm))
        _same(c, [u[i:i + 1] for u in a], (path, "alone", i))


# ---- 5. synchronised solve with rows ------------------------------------------------------------------------------------------------------------
def test_synced_solve_with_rows_vs_oracle_chain(M):
    """N = 13, 12 problems in four groups of three: pass 1 is the plain solve under the rows; pass 2 re-solves the faster members from the stretch
    of their pass-1 solutions with T fixed at the group's time, under the same rows"""
    path, nseg, sqp = "k_qp2_4", 4, 3
    x0, xf, rows, warm, ref, base = _parity_problems(M, 1, nseg)
    s = _solver(M, path, NPROB)
    s.set_bounds(rows)
    plain = s.solve(x0, xf, warm)
    group = (np.arange(NPROB) // 3).astype(np.int32)
    sx, su, sT, info, gT = s.solve_synced(x0, xf, group, warm, n_groups=4)
    elig = (plain[3]["status"] & HARD) == 0
    want = np.array([plain[2][elig & (group == g)].max() for g in range(4)])
    assert np.array_equal(gT, want)
    Tg = want[group]
    re_ = elig & (plain[2] < Tg)
    idx = list(np.nonzero(re_)[0])
    keep = np.nonzero(~re_)[0]
    assert len(idx) >= 4
    for a, p in zip((sx, su, sT), plain[:3]):
        assert np.array_equal(a[keep], p[keep])
    assert info[keep].tobytes() == plain[3][keep].tobytes()
    # the stretch of include/mpcmp.h (mpcmp_time_scale_batch) in NumPy, then the oracle's pass 2 under the row with [lbT, ubT] = [Tg, Tg]
    sc = plain[2] / Tg
    gx = plain[0].copy()
    gx[:, 1:-1, 7:] = plain[0][:, 1:-1, 7:] * sc[:, None, None]
    gx[:, 0], gx[:, -1] = x0, xf
    gu = plain[1] * (sc * sc)[:, None, None]
    ref2 = list(POOL.map(lambda b: o.solve(_ocfg(nseg, sqp, rows[b], lbT=Tg[b], ubT=Tg[b]), x0[b], xf[b], gx[b], gu[b], Tg[b]), idx))
    _check_solve((sx, su, sT, info), ref2, "pass 2 under rows", idx=idx)


# ---- 6. rows together with payload rows and final-time rows ------------------------------------------------------------------------------------
def test_rows_with_payload_rows_and_time_windows(M):
    """the three per-problem tables are independent: problem b under its bound row, with a payload of (b % 3) kg and a window whose lbT lies above
    its free final time for every second problem, against the oracle with all three in its arguments"""
    path, nseg, sqp = "k_qp2_4", 4, 3
    x0, xf, rows, warm, ref, base = _parity_problems(M, 1, nseg)
    s = _solver(M, path, NPROB)
    mass = (np.arange(NPROB) % 3).astype(np.float64)
    lbT = np.where(np.arange(NPROB) % 2 == 1, 1.2 * np.array([r[2] for r in ref]), 0.0)
    ubT = np.full(NPROB, 10.0)
    s.set_bounds(rows)
    s.set_payloads(mass)
    s.set_time_windows(lbT, ubT)
    got = s.solve(x0, xf, warm)
    tool = M.default_model().tool[:]
    models = [o.Model.from_buffer_copy(M.model_add_payload(M.default_model(), M.payload(mass[b], tool))) for b in range(NPROB)]
    want = list(POOL.map(lambda b: o.solve(_ocfg(nseg, sqp, rows[b], lbT=lbT[b], ubT=ubT[b]), x0[b], xf[b], warm[0][b], warm[1][b], warm[2][b],
                                           model=models[b]), range(NPROB)))
    _check_solve(got, want, "bounds + payload + window rows")
    assert sum(np.abs(want[b][0] - ref[b][0]).max() > 1e-3 for b in range(NPROB)) >= 6
    # each table clears on its own
    s.clear_payloads(); s.clear_time_windows()
    _check_solve(s.solve(x0, xf, warm), ref, "bound rows alone again")


# ---- 7. the device setter ----------------------------------------------------------------------------------------------------------------------
def test_set_bounds_device_equals_host(M):
    import torch
    path, nseg = "k_qp5_6", 6
    x0, xf, rows, warm, ref, base = _parity_problems(M, 1, nseg)
    s = _solver(M, path, NPROB)
    s.set_bounds(rows)
    host = s.solve(x0, xf, warm)
    s.clear_bounds()
    d = torch.from_numpy(np.frombuffer(rows.tobytes(), dtype=np.uint8).copy()).cuda()
    s.set_bounds_device(NPROB, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _same(s.solve(x0, xf, warm), host, "device setter")
    s.set_bounds_device(0, 0)
    assert s.bound_rows == 0
    _same(s.solve(x0, xf, warm), _solver(M, path, NPROB).solve(x0, xf, warm), "device clear")


# ---- 8. pose targets ---------------------------------------------------------------------------------------------------------------------------
def test_pose_targets_follow_the_rows(M):
    """the wrap, the choice and the flags follow the NumPy restatement of tests/test_gpu_pose_targets.py fed with each problem's own rows; one
    problem's only converged start lies inside the configuration's range but outside its narrow row: MPCMP_IK_Q_OUT_OF_BOUNDS; without rows the
    outputs are those of a context that never had any"""
    from mpc_motion_planner_amd import scenarios
    from test_gpu_pose_targets import _wrap, _choose, _poses, _host_runs
    B, S = 48, 8
    cfg = M.default_config(4, 3, margins=CTX_MARGINS)
    model = M.default_model()
    qt = scenarios.sample_states(B, (0.9, 0.9, 0.5, 0.9, 0.1), stream_offset=410)[:, :7]
    rng = np.random.default_rng(17)
    seeds = scenarios.ik_seeds(B, S, cfg)
    # problem 0: one start, next to a true configuration whose joint 0 sits at 0.85 of the physical range: inside the config's 0.9, outside the row's 0.8
    lim = M.default_limits()
    mid, half = 0.5 * (lim["qmax"][0] + lim["qmin"][0]), 0.5 * (lim["qmax"][0] - lim["qmin"][0])
    qt[0, 0] = mid + 0.85 * half
    R, p = _poses(M, model, qt)
    seeds[0, :] = qt[0] + 1e-3
    tw = np.concatenate([rng.uniform(-0.25, 0.25, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))], axis=1)
    rows = np.zeros(B, dtype=M.BOUNDS_DTYPE)
    for b in range(B):
        rows[b] = _row(M, ("narrow", "default", "slow", "narrow")[b % 4])
    s = M.Solver(cfg, B)
    xf0, info0 = s.pose_targets(R, p, seeds, twist=tw)
    s.set_bounds(rows)
    xf, info = s.pose_targets(R, p, seeds, twist=tw)
    assert info["status"][0] & M.IK_Q_OUT_OF_BOUNDS and not info0["status"][0] & (M.IK_Q_OUT_OF_BOUNDS | M.IK_NOT_CONVERGED)
    err1 = np.zeros((B, S)); its1 = np.zeros((B, S), dtype=int)
    for k in range(S):
        _, i1 = s.pose_targets(R, p, seeds[:, k:k + 1])
        err1[:, k], its1[:, k] = i1["err"], i1["iters"]
    ndiff = 0
    for b in range(B):
        lo, hi, lv, uv = rows["lbx"][b, :7], rows["ubx"][b, :7], rows["lbx"][b, 7:], rows["ubx"][b, 7:]
        qh, conv, its = _host_runs(M, model, R[b:b + 1], p[b:b + 1], seeds[b:b + 1], lo, hi)
        want = _choose(qh[0], conv[0], err1[b], lo, hi)
        if (its[0] != its1[b]).any() and info["seed"][b] != want:      # (a start whose host and device iteration counts differ: FMA contraction)
            ndiff += 1
            continue
        assert info["seed"][b] == want, (b, info["seed"][b], want)
        k = info["seed"][b]
        assert np.abs(xf[b, :7] - qh[0, k]).max() <= 1e-8, b
        inb = bool(np.all((qh[0, k] >= lo) & (qh[0, k] <= hi)))
        assert bool(info["status"][b] & M.IK_Q_OUT_OF_BOUNDS) == (not inb), b
        out = bool(((xf[b, 7:] < lv) | (xf[b, 7:] > uv)).any())
        assert bool(info["status"][b] & M.IK_QD_OUT_OF_BOUNDS) == out, b
    assert ndiff <= 1
    slow = np.arange(B) % 4 == 2
    assert (info["status"][slow] & M.IK_QD_OUT_OF_BOUNDS).sum() >= (info0["status"][slow] & M.IK_QD_OUT_OF_BOUNDS).sum()
    # more problems than rows; and back to no rows
    s.set_bounds(rows[:B - 1])
    with pytest.raises(M.MpcmpError) as e:
        s.pose_targets(R, p, seeds)
    assert e.value.code == -1 and "bound rows" in str(e.value)
    s.clear_bounds()
    _same(s.pose_targets(R, p, seeds, twist=tw), (xf0, info0), "pose targets after a clear")
    _same(M.Solver(cfg, B).pose_targets(R, p, seeds, twist=tw), (xf0, info0), "pose targets of a fresh context")


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_errors(M):
    """each rejection leaves the outputs and the table untouched"""
    B = 8
    x0, xf, rows = _problems(M, 1, B, 60)
    s = M.Solver(M.default_config(4, 2, margins=CTX_MARGINS), B)
    warm = s.warm_start(x0, xf)
    plain = s.solve(x0, xf, warm)

    def einval(fn, *a, **k):
        with pytest.raises(M.MpcmpError) as e:
            fn(*a, **k)
        assert e.value.code == -1, str(e.value)
        return str(e.value)

    # n outside [1, max_batch]
    einval(s.set_bounds, np.zeros(B + 1, dtype=M.BOUNDS_DTYPE))
    assert M.lib().mpcmp_set_bounds(s._ctx, -1, rows.ctypes.data) == -1 and M.lib().mpcmp_set_bounds(s._ctx, 0, rows.ctypes.data) == -1
    assert M.lib().mpcmp_set_bounds(s._ctx, 3, None) == -1
    _same(s.solve(x0, xf, warm), plain, "no rows after the rejected counts")
    # more problems than rows: nothing is written, the rows stay
    s.set_bounds(rows[:B - 1])
    under = s.solve(x0[:B - 1], xf[:B - 1], tuple(w[:B - 1] for w in warm))
    out = [np.full_like(a, -7.0) for a in plain[:3]]
    assert "bound rows" in einval(s.solve, x0, xf, warm)
    einval(s.warm_start, x0, xf)
    einval(s.qp, x0, xf, *warm)
    einval(s.solve_synced, x0, xf, np.zeros(B, dtype=np.int32), warm)
    import ctypes as C
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert M.lib().mpcmp_solve_batch(s._ctx, B, vp(x0), vp(xf), None, None, None, vp(out[0]), vp(out[1]), vp(out[2]), None) == -1
    assert all((a == -7.0).all() for a in out)
    # bad rows, each kind: the row and the field are named, nothing changes (the B - 1 rows stay in force)
    for field, i, lb, ub in (("lbx", 3, np.nan, 1.0), ("ubu", 2, -1.0, np.nan), ("lbg", 5, 2.0, 1.0), ("lbx", 9, np.inf, np.inf),
                             ("ubg", 0, -np.inf, -np.inf), ("lbg", 7, 0.3, 0.3 + 5e-5)):
        bad = rows.copy()
        bad["l" + field[1:]][4, i], bad["u" + field[1:]][4, i] = lb, ub
        msg = einval(s.set_bounds, bad)
        assert "row 4" in msg and "%s[%d]" % (field if field[0] == "l" else "l" + field[1:], i) in msg, msg
        _same(s.solve(x0[:B - 1], xf[:B - 1], tuple(w[:B - 1] for w in warm)), under, ("rows as before", field))
        einval(s.solve, x0, xf, warm)
    # the narrow general row is accepted at num_seg 6 (k_qp5 / k_qp3 assemble its rho_eq)
    s6 = M.Solver(M.default_config(6, 2, margins=CTX_MARGINS), B)
    ok = rows.copy()
    ok["lbg"][4, 7], ok["ubg"][4, 7] = 0.3, 0.3 + 5e-5
    s6.set_bounds(ok)
    # mpcmp_set_config keeps working with rows set, and the rows win for the six tables
    s.set_config(M.default_config(4, 2, margins=(0.5, 0.5, 0.5, 0.5)))
    _same(s.solve(x0[:B - 1], xf[:B - 1], tuple(w[:B - 1] for w in warm))[:3], under[:3], "rows win over a new configuration")
    s.set_config(M.default_config(4, 2, margins=CTX_MARGINS))
    # the receding-horizon driver: rows set -> mpcmp_rh_init refuses; a loop running -> the setters refuse
    s.set_bounds(rows)
    assert "receding-horizon" in einval(s.rh_init, x0, xf)
    s.clear_bounds()
    _same(s.solve(x0, xf, warm), plain, "after the rejections and a clear")
    s.rh_init(x0, xf)
    assert "receding-horizon" in einval(s.set_bounds, rows)
    einval(s.set_bounds_device, B, 1, 0)
