"""Oracle parity away from mpcmp_default_config: every QP loop kernel and the step kernels read mpcmp_config at run time, so each solver setting
(test period and iteration cap, tolerances, ADMM parameters, line search, degenerate and infinite bounds) is crossed with every kernel path and
compared with the oracle (oracle/ocp.c).  Every case first proves on the oracle that it changes the answer, so a setting that stops mattering fails
its case instead of passing it.  Run with -m gpu."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as o

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
INF = float("inf")
XCH_STRIDE = 1024                     # MPCMP_XCH_STRIDE: doubles per arm and OCP in the two-arm exchange slots

# kernel paths: (id, num_seg, arms, environment at mpcmp_create, loop kernel reported by mpcmp_kernel_timing)
PATHS = [("k_qp1", 1, 1, {}, "k_qp"),
         ("k_qp2_2", 2, 1, {}, "k_qp2"), ("k_qp_2_v1", 2, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp2_4", 4, 1, {}, "k_qp2"), ("k_qp3_4", 4, 1, {"MPCMP_QP13": "3"}, "k_qp3"), ("k_qp_4_v1", 4, 1, {"MPCMP_FORCE_V1": "1"}, "k_qp"),
         ("k_qp5_6", 6, 1, {}, "k_qp5"), ("k_qp3_6", 6, 1, {"MPCMP_QP19": "3"}, "k_qp3"),
         ("k_qp3_8", 8, 1, {}, "k_qp3"),
         ("k_qp3_6x2", 6, 2, {}, "k_qp3"), ("k_qp3_8x2", 8, 2, {}, "k_qp3")]
PATH = {p[0]: p for p in PATHS}

# problems (scenario stream offsets) whose QP, linearised at an 8-iteration SQP solution, converges under the default settings: only there do the
# test period and the tolerances decide the answer (from the start guess nearly every QP runs into the 700-iteration cap)
OFFSETS = {(1, 1): (1, 4, 9), (1, 2): (2, 7, 10), (1, 4): (2, 7, 8), (1, 6): (2, 8), (1, 8): (2, 8), (2, 6): (5, 8), (2, 8): (8, 10)}

LOCK_J, LOCK_C = 0, 0.25              # the locked joint (base yaw: a value inside its box for both arms) and where it is locked


def _lock(c):
    c.lbx[LOCK_J] = c.ubx[LOCK_J] = LOCK_C
    c.lbx[7 + LOCK_J] = c.ubx[7 + LOCK_J] = 0.0
    c.lbu[LOCK_J] = c.ubu[LOCK_J] = 0.0


def _narrow_boxes(w):
    """a velocity box and an acceleration box of width w (kept well away from the 1e-4 of the rho rule on both sides)"""
    def f(c):
        c.lbx[7 + 5], c.ubx[7 + 5] = -w / 2, w / 2
        c.lbu[1], c.ubu[1] = -w / 2, w / 2
    return f


def _narrow_row(w):
    """a torque row of width w"""
    def f(c):
        c.lbg[2], c.ubg[2] = -w / 2, w / 2
    return f


def _tau_off(c):
    for j in range(7):
        c.lbg[j], c.ubg[j] = -INF, INF


def _min_height_off(c):
    c.lbg[7] = -INF


def _lin_low_wrist(narm, lx, lu, lT):
    """interior nodes at q_2 = 1.5, q_4 = -1.0 (every arm): the joint-7 origin sits at z = -0.065, below the 0.05 of the height row"""
    lx = lx.copy()
    for a in range(narm):
        lx[:, 1:-1, 7 * a + 1] = 1.5
        lx[:, 1:-1, 7 * a + 3] = -1.0
    return lx, lu, lT


# linearisation points of the infinite-bound cases: at the default one the finite bound is inactive and switching it off changes nothing, so these
# cases move the point to where it binds (torque rows: four times the accelerations; min height: the wrist below the table; ubT: T = 12 > 10)
LIN = {"torque_rows_off": lambda narm, lx, lu, lT: (lx, 4.0 * lu, lT), "min_height_off": _lin_low_wrist,
       "ubT_inf": lambda narm, lx, lu, lT: (lx, lu, np.full_like(lT, 12.0))}

FIXED_T = dict(lbT=2.5, ubT=2.5)
LS_FIXED_T = dict(lbT=1.0, ubT=1.0)       # (a final time the 3-iteration solves of every path's problems backtrack to alpha = 2^-9 on)
# settings cases: fields set on top of the MARGINS configuration (fn: a function that edits the bound tables)
CASES = {
    "check_every_1": dict(check_every=1), "check_every_7": dict(check_every=7), "check_every_40": dict(check_every=40),
    "qp_iters_24": dict(qp_iters=24), "qp_iters_60": dict(qp_iters=60), "qp_iters_113": dict(qp_iters=113),
    "check_every_7_qp_iters_60": dict(check_every=7, qp_iters=60),
    "eps_1e-5": dict(eps_abs=1e-5, eps_rel=1e-5), "eps_abs_1e-2_rel_0": dict(eps_abs=1e-2, eps_rel=0.0),
    "rho_0.005": dict(rho=0.005), "rho_0.1": dict(rho=0.1), "sigma_1e-4": dict(sigma=1e-4), "alpha_1.0": dict(alpha=1.0), "alpha_1.8": dict(alpha=1.8),
    "rho_eq_scale_1": dict(rho_eq_scale=1.0), "rho_eq_scale_1e4": dict(rho_eq_scale=1e4),
    "hess_reg_1e-6": dict(hess_reg=1e-6), "hess_reg_0.1": dict(hess_reg=0.1),
    "eps_target_0": dict(eps_target=0.0), "eps_target_0.05": dict(eps_target=0.05), "fixed_T": dict(FIXED_T),
    "locked_joint": dict(fn=_lock), "box_5e-5": dict(fn=_narrow_boxes(5e-5)), "box_2e-4": dict(fn=_narrow_boxes(2e-4)),
    "row_5e-5": dict(fn=_narrow_row(5e-5)), "row_2e-4": dict(fn=_narrow_row(2e-4)),
    "torque_rows_off": dict(fn=_tau_off), "min_height_off": dict(fn=_min_height_off), "ubT_inf": dict(ubT=INF),
}
# a general row narrower than 1e-4 takes rho_eq; the assembly of k_qp and k_qp2 gives every general row the plain rho, so num_seg 1, 2, 4 reject
# such a row (validate(), mpcmp.hip) and the case runs from num_seg 6 on
NARROW_ROW_MIN_NSEG = 6
QP_PARAMS = [(p[0], c) for p in PATHS for c in CASES if c != "row_5e-5" or p[1] >= NARROW_ROW_MIN_NSEG]
# cases the step kernels read: checked by a 3-iteration solve.  The line-search settings only matter where the search backtracks: on the
# fixed-T problem (the default bounds accept alpha = 1)
SOLVE_CASES = {
    "ls_iters_2": dict(LS_FIXED_T, ls_iters=2), "ls_iters_3": dict(LS_FIXED_T, ls_iters=3), "ls_iters_5": dict(LS_FIXED_T, ls_iters=5),
    "ls_eta_0.1": dict(FIXED_T, ls_eta=0.1), "ls_tau_0.7": dict(LS_FIXED_T, ls_tau=0.7), "quirk_dtau_dT_0": dict(quirk_dtau_dT=0),
    "hess_reg_1e-6": CASES["hess_reg_1e-6"], "hess_reg_0.1": CASES["hess_reg_0.1"], "eps_target_0": CASES["eps_target_0"],
    "eps_target_0.05": CASES["eps_target_0.05"], "locked_joint": CASES["locked_joint"], "fixed_T": CASES["fixed_T"],
}
# the answer a solve case must differ from: the defaults, or the fixed-T problem with the default line search for the line-search settings
SOLVE_BASE = {k: (LS_FIXED_T if k.startswith("ls_") else None) for k in SOLVE_CASES}
# ls_eta: at T = 1 every search runs to its last step whatever the Armijo fraction, so it runs at T = 2.5, where the searches stop part way; there
# 0.1 instead of 0.25 changes the oracle's answer on the problems of num_seg 1, 4 and 8 (one arm) only, so it runs on those paths
SOLVE_BASE["ls_eta_0.1"] = FIXED_T
SOLVE_PARAMS = [(p[0], c) for p in PATHS for c in SOLVE_CASES if c != "ls_eta_0.1" or (p[2] == 1 and p[1] in (1, 4, 8))]
# the Gershgorin shift is all the regularisation the Hessian has: at hess_reg = 1e-6 the KKT matrices are 1e3 times worse conditioned than at the
# default, and the kernels' and the oracle's factorisation orders (block inverses vs skyline Cholesky) end three SQP iterations 1e-6 apart in x
# (measured: 1.03e-6 at N = 4) with identical iteration counts, status words and step lengths.  The state tolerance of that case is 1e-5
SOLVE_X_TOL = {"hess_reg_1e-6": 1e-5}
# (a few cases per path: set_config must equal a context created with the configuration)
FRESH_CASES = ("check_every_7", "rho_eq_scale_1e4", "box_5e-5", "row_2e-4")


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _max_qp_iters(check_every):
    """largest qp_iters the two-arm exchange slots hold: 8 + qp_iters + 1 + 8 (qp_iters / check_every + 1) <= XCH_STRIDE"""
    q = 1
    while 8 + (q + 1) + 1 + 8 * ((q + 1) // check_every + 1) <= XCH_STRIDE:
        q += 1
    return q


def _config(nseg, narm, sqp, fields):
    import mpc_motion_planner_amd as M
    c = M.default_config(nseg, sqp, margins=MARGINS)
    for k, v in (fields or {}).items():
        if k == "fn":
            v(c)
        else:
            setattr(c, k, v)
    if narm == 2:      # (two arms: a cap beyond the exchange slots is rejected; such a case runs at the largest cap they hold)
        c.qp_iters = min(c.qp_iters, _max_qp_iters(c.check_every))
    return c


def _ocfg(cfg):
    return o.Config.from_buffer_copy(bytes(cfg))


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


def _create(M, path, cfg, B):
    _, nseg, narm, env, _ = PATH[path]
    with _env(env):             # the kernel choice is read at mpcmp_create only
        return M.Solver(cfg, B, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)


_CTX = {}


def _ctx(M, path):
    """one context per path for the whole module; cases move it with set_config"""
    if path not in _CTX:
        _, nseg, narm, _, kname = PATH[path]
        s = _create(M, path, M.default_config(nseg, 1, margins=MARGINS), 3)
        assert s.kernel_timing()[0] == kname, (path, s.kernel_timing()[0])
        _CTX[path] = s
    return _CTX[path]


def _omodels(narm):
    return o.arm_models(o.DUAL_BASES) if narm == 2 else None


def _osolve(narm, ocfg, x0, xf, wx, wu, wT):
    if narm == 1:
        return o.solve(ocfg, x0, xf, wx, wu, wT)
    return o.solve_multi(_omodels(narm), ocfg, x0, xf, wx, wu, wT)


def _limits():
    lim = o.default_limits()
    return MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]


_PROB = {}


def _problems(narm, nseg, locked):
    """(x0, xf, start guess, linearisation point) of the path's problems; the locked-joint case holds joint LOCK_J of every arm at LOCK_C, at rest.
    Start guess: the oracle's (one arm: the built-in warm start; two arms: the jerk-limited generator with the unlocked limits — it rejects a
    zero velocity limit by design, and the locked joint does not move).  Linearisation point: an 8-iteration oracle solve from it under the
    defaults, end states re-pinned (motionPlanner.cpp:199-207)."""
    key = (narm, nseg, locked)
    if key not in _PROB:
        from mpc_motion_planner_amd import scenarios
        offs = OFFSETS[(narm, nseg)]
        tables = dict(model=o.default_model(), limits=o.default_limits())     # (the oracle's, the same numbers as the library's: tests/test_ocp_reference_host.py builds these problems without the GPU library)
        x0, xf = [], []
        for off in offs:
            a0, af = scenarios.make_batch(1, MARGINS, stream_offset=off, **tables)
            if narm == 2:
                b0, bf = scenarios.make_batch(1, MARGINS, stream_offset=off + 7919, **tables)
                a0, af = o.merge_arm_states([a0[0], b0[0]])[None], o.merge_arm_states([af[0], bf[0]])[None]
            x0.append(a0[0]); xf.append(af[0])
        x0, xf = np.array(x0), np.array(xf)
        nq = 7 * narm
        if locked:
            for x in (x0, xf):
                x[:, [7 * a + LOCK_J for a in range(narm)]] = LOCK_C
                x[:, [nq + 7 * a + LOCK_J for a in range(narm)]] = 0.0
        deep = o.default_config(nseg, 8, margins=MARGINS)
        warm, lin = [], []
        for b in range(len(x0)):
            w = o.warm_start(deep, x0[b], xf[b]) if narm == 1 else o.warm_start_jerk_multi(nseg, *_limits(), x0[b], xf[b])
            xs, us, T, _ = _osolve(narm, deep, x0[b], xf[b], *w)
            g = xs.copy(); g[0] = x0[b]; g[-1] = xf[b]
            warm.append(w); lin.append((g, us, T))
        stack = lambda L: tuple(np.array([t[i] for t in L]) for i in range(3))
        _PROB[key] = (x0, xf, stack(warm), stack(lin))
    return _PROB[key]


_ORC = {}


def _qp_point(narm, nseg, case):
    """(x0, xf, linearisation point) of the case's QPs: the locked-joint problems for that case, moved by LIN for the infinite-bound cases"""
    x0, xf, _, lin = _problems(narm, nseg, case == "locked_joint")
    return (x0, xf) + (LIN[case](narm, *lin) if case in LIN else lin)


def _oracle_qp(narm, nseg, case, fields, point=None):
    """the oracle's answer to the QP with settings `fields` at the linearisation point of case `point` (default: `case`): one arm (p, y, iterations)
    of orc_debug_qp; two arms (xs, us, T, info) of a one-iteration solve, the form mpcmp_qp_batch has no two-arm counterpart of.  Cached: paths of
    one discretisation share it"""
    point = case if point is None else point
    key = ("qp", narm, nseg, case, point)
    if key not in _ORC:
        x0, xf, lx, lu, lT = _qp_point(narm, nseg, point)
        ocfg = _ocfg(_config(nseg, narm, 1, fields))
        if narm == 1:
            _ORC[key] = [o.debug_qp(ocfg, x0[b], xf[b], lx[b], lu[b], lT[b]) for b in range(len(x0))]
        else:
            _ORC[key] = [_osolve(narm, ocfg, x0[b], xf[b], lx[b], lu[b], lT[b]) for b in range(len(x0))]
    return _ORC[key]


def _oracle_solve(narm, nseg, case, fields, base=False):
    key = ("solve", narm, nseg, case, base)
    if key not in _ORC:
        x0, xf, (wx, wu, wT), _ = _problems(narm, nseg, case == "locked_joint")
        ocfg = _ocfg(_config(nseg, narm, 3, fields))
        _ORC[key] = [_osolve(narm, ocfg, x0[b], xf[b], wx[b], wu[b], wT[b]) for b in range(len(x0))]
    return _ORC[key]


def _differs_qp(narm, a, b):
    """non-vacuity: iteration count, or the step by more than 1e-6"""
    if narm == 1:
        return any(ra[2] != rb[2] or np.abs(ra[0] - rb[0]).max() > 1e-6 for ra, rb in zip(a, b))
    return any(ra[3].qp_iters_total != rb[3].qp_iters_total or np.abs(ra[0] - rb[0]).max() > 1e-6 or abs(ra[2] - rb[2]) > 1e-6 for ra, rb in zip(a, b))


def _run_qp(M, s, narm, nseg, case):
    x0, xf, lx, lu, lT = _qp_point(narm, nseg, case)
    if narm == 1:
        return s.qp(x0, xf, lx, lu, lT)
    return s.solve(x0, xf, (lx, lu, lT))


def _check_qp(narm, got, ref, what):
    if narm == 1:
        p, y, it = got
        for b, (p0, y0, it0) in enumerate(ref):
            assert it[b] == it0, (what, b, it[b], it0)
            assert np.abs(p[b] - p0).max() <= 1e-7 * (1 + np.abs(p0).max()), (what, b, np.abs(p[b] - p0).max())
            assert np.abs(y[b] - y0).max() <= 1e-6 * (1 + np.abs(y0).max()), (what, b, np.abs(y[b] - y0).max())
    else:
        _check_solve(got, ref, what, alpha=False)


def _check_solve(got, ref, what, alpha=True, x_tol=1e-6):
    sx, su, sT, info = got
    for b, (xs, us, T, oi) in enumerate(ref):
        assert info["status"][b] == oi.status and info["qp_iters_total"][b] == oi.qp_iters_total and info["qp_capped"][b] == oi.qp_capped, \
            (what, b, info["status"][b], oi.status, info["qp_iters_total"][b], oi.qp_iters_total)
        if alpha:
            assert info["last_alpha"][b] == oi.last_alpha, (what, b, info["last_alpha"][b], oi.last_alpha)
        assert abs(sT[b] - T) <= 1e-6 * abs(T), (what, b, sT[b], T)
        assert np.abs(sx[b] - xs).max() <= x_tol, (what, b, np.abs(sx[b] - xs).max())
        assert np.abs(su[b] - us).max() <= 1e-5, (what, b, np.abs(su[b] - us).max())


# ---- QP check: every path x every settings case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,case", QP_PARAMS)
def test_qp_settings_vs_oracle(M, path, case):
    """one QP per problem (two arms: a one-iteration solve) under the case's settings, moved in with set_config: identical ADMM iteration counts,
    p <= 1e-7 (1 + |p|), y <= 1e-6 (1 + |y|) (two arms: states, final time, iteration counts, capped QPs and status words as a solve); and the
    oracle's answer under the case differs from its answer under the defaults"""
    _, nseg, narm, _, kname = PATH[path]
    fields = CASES[case]
    ref = _oracle_qp(narm, nseg, case, fields)
    dflt = _oracle_qp(narm, nseg, "default", None, point=case)       # (the defaults on the same problems at the same point)
    assert _differs_qp(narm, ref, dflt), (path, case, "the setting does not change the oracle's answer")
    s = _ctx(M, path)
    cfg = _config(nseg, narm, 1, fields)
    s.set_config(cfg)
    try:
        got = _run_qp(M, s, narm, nseg, case)
    finally:
        s.set_config(M.default_config(nseg, 1, margins=MARGINS))
    _check_qp(narm, got, ref, (path, case))
    assert s.kernel_timing()[0] == kname
    if case in FRESH_CASES:             # set_config == a context created with the configuration, bit for bit
        fresh = _run_qp(M, _create(M, path, cfg, 3), narm, nseg, case)
        for a, b in zip(got, fresh):
            assert np.array_equal(a, b), (path, case)


@pytest.mark.parametrize("path", [p[0] for p in PATHS if p[1] < NARROW_ROW_MIN_NSEG])
def test_narrow_general_row_rejected_below_num_seg_6(M, path):
    """k_qp / k_qp2 paths: a torque row narrower than 1e-4 is rejected by mpcmp_create and by set_config, and the context keeps working"""
    _, nseg, narm, _, _ = PATH[path]
    cfg = _config(nseg, narm, 1, CASES["row_5e-5"])
    with pytest.raises(M.MpcmpError) as e:
        _create(M, path, cfg, 1)
    assert e.value.code == -1 and "lbg" in str(e.value)
    s = _ctx(M, path)
    with pytest.raises(M.MpcmpError) as e:
        s.set_config(cfg)
    assert e.value.code == -1 and "lbg" in str(e.value)
    ref = _oracle_qp(narm, nseg, "default", None)
    _check_qp(narm, _run_qp(M, s, narm, nseg, "default"), ref, (path, "after the rejection"))


# ---- solve check: the settings the step kernels read ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,case", SOLVE_PARAMS)
def test_solve_settings_vs_oracle(M, path, case):
    """3 SQP iterations from the start guess: status words, ADMM iteration counts, capped QPs and last step lengths equal; |dT| <= 1e-6 T,
    x <= 1e-6, u <= 1e-5; and the oracle's answer differs from the one without the setting"""
    _, nseg, narm, _, kname = PATH[path]
    fields = SOLVE_CASES[case]
    ref = _oracle_solve(narm, nseg, case, fields)
    bname = SOLVE_BASE[case]
    base = _oracle_solve(narm, nseg, case, bname, base=True)
    assert any(a[3].qp_iters_total != b[3].qp_iters_total or a[3].last_alpha != b[3].last_alpha or np.abs(a[0] - b[0]).max() > 1e-6
               for a, b in zip(ref, base)), (path, case, "the setting does not change the oracle's answer")
    x0, xf, warm, _ = _problems(narm, nseg, case == "locked_joint")
    s = _ctx(M, path)
    s.set_config(_config(nseg, narm, 3, fields))
    try:
        got = s.solve(x0, xf, warm)
    finally:
        s.set_config(M.default_config(nseg, 1, margins=MARGINS))
    _check_solve(got, ref, (path, case), x_tol=SOLVE_X_TOL.get(case, 1e-6))
    if case.startswith("ls_"):          # (the line search did backtrack)
        assert any(oi.last_alpha < 1 for *_, oi in ref)


# ---- two arms: the exchange slots filled to the last one --------------------------------------------------------------------------------
@pytest.mark.parametrize("check_every,qp_iters", [(7, 471), (25, 767), (40, 839)])
@pytest.mark.parametrize("path", ["k_qp3_6x2", "k_qp3_8x2"])
def test_exchange_slots_full_vs_oracle(M, path, check_every, qp_iters):
    """eps_abs = eps_rel = 0: every QP runs to its cap, the largest one the slots hold for the test period; one more is rejected by
    mpcmp_create_multi and by set_config"""
    _, nseg, narm, _, _ = PATH[path]
    assert qp_iters == _max_qp_iters(check_every)
    fields = dict(eps_abs=0.0, eps_rel=0.0, check_every=check_every, qp_iters=qp_iters)
    case = "xch_%d_%d" % (check_every, qp_iters)
    ref = _oracle_qp(narm, nseg, case, fields)
    assert all(oi.qp_iters_total == qp_iters and oi.qp_capped == 1 for *_, oi in ref)
    assert _differs_qp(narm, ref, _oracle_qp(narm, nseg, "default", None, point=case))
    s = _ctx(M, path)
    cfg = _config(nseg, narm, 1, fields)
    s.set_config(cfg)
    try:
        got = _run_qp(M, s, narm, nseg, case)
        _check_qp(narm, got, ref, (path, case))
        over = _config(nseg, narm, 1, fields)
        over.qp_iters = qp_iters + 1                  # (after _config, which would clamp it)
        with pytest.raises(M.MpcmpError) as e:
            s.set_config(over)
        assert e.value.code == -1 and "exchange slots" in str(e.value)
    finally:
        s.set_config(M.default_config(nseg, 1, margins=MARGINS))
    ctx = C.c_void_p()
    assert M.lib().mpcmp_create_multi(C.byref(over), M.arm_models(M.DUAL_BASES), 2, 0, 1, C.byref(ctx)) == -1
    fresh = _run_qp(M, _create(M, path, cfg, 3), narm, nseg, case)
    for a, b in zip(got, fresh):
        assert np.array_equal(a, b)


# ---- eval_constraints without the d tau / dT quirk ----------------------------------------------------------------------------------------
def test_eval_constraints_quirk_off_vs_oracle(M):
    cfg = M.default_config(4, 1, margins=MARGINS, quirk_dtau_dT=0)
    s = M.Solver(cfg, 8)
    rng = np.random.default_rng(11)
    lim = o.default_limits()
    for nn in (1, 13, 40):                                     # below, equal to and above one node chunk
        x = np.concatenate([rng.uniform(lim["qmin"], lim["qmax"], (nn, 7)), rng.uniform(-1, 1, (nn, 7)) * lim["vmax"]], axis=1)
        u = rng.uniform(-1, 1, (nn, 7)) * lim["amax"]
        g, G = s.eval_constraints(x, u)
        for i in range(nn):
            g0, G0 = o.eval_constraints(x[i], u[i], quirk=0)
            assert np.abs(g[i] - g0).max() < 1e-11
            assert np.abs(G[i] - G0).max() < 1e-10 * (1 + np.abs(G0).max())
            assert np.abs(G0 - o.eval_constraints(x[i], u[i], quirk=1)[1]).max() > 1e-3       # (the flag changes the Jacobian)


# ---- receding horizon: the arrival rule reads eps_target ------------------------------------------------------------------------------------
def test_receding_horizon_arrival_eps_target_vs_oracle(M):
    """eps_target = 0.05 at N = 13: k_advance's arrival rule and the terminal box both read it.  rh_run(1) repeated: after every step the ARRIVED
    bits, states and iteration counts equal the oracle chain's with the same setting, and the arrival steps differ from the default's"""
    from mpc_motion_planner_amd import scenarios
    kw = dict(eps_target=0.05)
    cfg = M.default_config(4, 2, margins=MARGINS, **kw)
    ocfg = o.default_config(4, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1, **kw)
    B, steps, dt = 6, 33, 0.1          # (0.05 instead of 0.01: instance 0 arrives one step earlier, instance 3 at step 18 instead of never)
    x0, xf = scenarios.make_batch(B, stream_offset=900)
    ch = o.rh_chain(ocfg, x0, xf, steps, dt)
    ch0 = o.rh_chain(o.default_config(4, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1), x0, xf, steps, dt)
    assert ch["retired"].all() and not np.array_equal(ch["retired_at"], ch0["retired_at"]), (ch["retired_at"], ch0["retired_at"])
    s = M.Solver(cfg, B)
    s.rh_init(x0, xf)
    for k in range(steps):
        s.rh_run(1, dt, use_graph=False)
        xg, sx, su, sT, info = s.rh_get()
        ret = ch["hist_retired"][k]
        assert np.array_equal((info["status"] & M.STATUS_ARRIVED) != 0, ret), (k, info["status"], ret)
        assert np.array_equal(info["qp_iters_total"], ch["hist_its"][k]), (k, info["qp_iters_total"], ch["hist_its"][k])
        assert np.abs(xg - ch["hist_x"][k]).max() < 1e-6, (k, np.abs(xg - ch["hist_x"][k]).max())
        assert s.rh_stats() == (ch["hist_n_solves"][k], int(ret.sum()))
