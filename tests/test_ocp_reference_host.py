"""The dense reference of the OCP / QP / SQP layer (tests/ocp_reference.py) against itself and against the oracle (oracle/ocp.c), on the CPU.

  - its Jacobian and Hessian arrow against central differences of its own constraint functions in long double;
  - its float64 against its long double: the rounding floor every bar of oracle against reference is 100 times of;
  - the oracle's QPs (orc_debug_qp, orc_debug_qp_multi) against the dense ADMM: iteration counts, p, y; the epsilon-KKT certificate on the oracle's (p, y);
  - the oracle's SQP (orc_solve, orc_solve_multi) against sqp(): iterate and result record.
The problems are those of tests/test_gpu_solver_settings.py (OFFSETS); every case asserts that none of its termination tests and Armijo tests is
a near tie, so that equal iteration counts and step lengths are a fair demand."""
import numpy as np
import pytest

import ocp_reference as R
import oracle_py as o
import test_gpu_solver_settings as S
from test_gpu_solver_settings import MARGINS, OFFSETS

LD = np.longdouble
TERMINATION_MARGIN, ARMIJO_MARGIN = 1e-6, 1e-9          # smallest relative distance of a termination / Armijo test from its threshold


def _real(nseg):
    return LD if nseg <= 4 else np.float64


def _problems(narm, nseg):
    """[(x0, xf, start guess, linearisation point)] of test_gpu_solver_settings._problems, problem by problem: the problems the GPU tests run"""
    x0, xf, warm, lin = S._problems(narm, nseg, False)
    return [(x0[b], xf[b], tuple(a[b] for a in warm), tuple(a[b] for a in lin)) for b in range(len(x0))]


def _models(narm):
    return o.arm_models(o.DUAL_BASES) if narm == 2 else None


def _osolve(narm, cfg, x0, xf, w):
    return o.solve(cfg, x0, xf, *w) if narm == 1 else o.solve_multi(_models(narm), cfg, x0, xf, *w)


def _cfg(nseg, sqp_iters=1, **kw):
    return o.default_config(nseg, sqp_iters, margins=MARGINS, **kw)


# QP cases of one problem: (name, linearisation point, settings, warm multipliers?)
SHORT = dict(qp_iters=3, check_every=1)
QP_CASES = [("start", "warm", {}), ("lin", "lin", {}), ("start_short", "warm", SHORT), ("lin_short", "lin", SHORT)]

_QP = {}


def _ref_qp(narm, nseg, b, case, real):
    """the reference's QP of problem b and its ADMM run: (Q, p, y, iterations, capped, trace), cached.  Case "lin_warm": the convergent point,
    qp_warm_start = 1, multipliers = 0.7 times the duals of case "lin" (non-zero, and not the answer itself)"""
    key = (narm, nseg, b, case, real)
    if key not in _QP:
        x0, xf, w, lin = _problems(narm, nseg)[b]
        if case == "lin_warm":
            cfg, pt = _cfg(nseg, qp_warm_start=1), lin
            lam = 0.7 * _ref_qp(narm, nseg, b, "lin", real)[2]
        else:
            _, where, kw = next(c for c in QP_CASES if c[0] == case)
            cfg, pt, lam = _cfg(nseg, **kw), (w if where == "warm" else lin), None
        P = R.Problem(cfg, _models(narm), x0, xf, real)
        Q = P.qp(P.pack(*pt), lam)
        _QP[key] = (Q,) + R.admm(cfg, Q, lam) + (cfg, pt, lam)
    return _QP[key]


_SQP = {}


def _ref_sqp(narm, nseg, b, real):
    key = (narm, nseg, b, real)
    if key not in _SQP:
        x0, xf, w, _ = _problems(narm, nseg)[b]
        _SQP[key] = R.sqp(_cfg(nseg, 3), _models(narm), x0, xf, w, real=real)
    return _SQP[key]


def _rel(a, b):
    """largest difference relative to 1 + the largest entry of b"""
    return float(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).max() / (1 + np.abs(b).max()))


def _abs(a, b):
    return float(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)).max())


# ---- grid -------------------------------------------------------------------------------------------------------------------------------------
def test_nodes_and_differentiation_matrix():
    """the barycentric D differentiates cubics exactly at the local nodes, and equals the oracle's; so do the node times"""
    D, xi = R.diff_matrix(LD), R.local_nodes(LD)
    for coef in ([1, 0, 0, 0], [0.3, -1, 0, 0], [0, 0.5, 2, 0], [-0.7, 0.2, -1.1, 0.9]):
        c = np.array(coef, dtype=LD)
        val = sum(c[k] * xi ** k for k in range(4))
        der = sum(k * c[k] * xi ** (k - 1) for k in range(1, 4))
        assert np.abs(D @ val - der).max() < 1e-17
    assert np.abs(R.diff_matrix() - o.diff_matrix()).max() < 1e-14
    for nseg in (1, 2, 4, 6, 8):
        t = R.nodes(nseg)
        assert len(t) == 3 * nseg + 1 and np.all(np.diff(t) > 0) and t[0] == 0 and t[-1] == 1
        assert np.abs(t - o.time_nodes(nseg)).max() < 1e-15


# ---- Jacobian and Hessian against differences -----------------------------------------------------------------------------------------------------
def _richardson(F, z, cols, h):
    """d F / d z[cols] [rows, len(cols)] by central differences at h and h / 2 in long double, Richardson-extrapolated to fourth order, and the
    estimate |fourth-order level - second-order level at h / 2| (the manner of rbd_reference.Reference.dtau_dq)"""
    E = np.zeros((len(cols), len(z)), dtype=LD)
    E[np.arange(len(cols)), cols] = 1
    h = LD(h)
    Z = np.concatenate([z + h * E, z - h * E, z + h / 2 * E, z - h / 2 * E])
    f = F(Z)
    nc = len(cols)
    D1 = (f[:nc] - f[nc:2 * nc]) / (2 * h)
    D2 = (f[2 * nc:3 * nc] - f[3 * nc:]) / h
    Rr = (4 * D2 - D1) / 3
    return Rr.T, np.abs(Rr - D2).T.astype(np.float64)


JAC_CASES = [(1, 1, None), (1, 4, None), (2, 6, (0, 7, 18))]        # (arms, num_seg, nodes whose columns are differenced: None = every column)


@pytest.mark.parametrize("narm,nseg,at", JAC_CASES)
def test_jacobian_and_hessian_vs_differences(narm, nseg, at):
    """A's dynamics and path blocks = central differences of defects() and path_values() (long double, Richardson, entry by entry within
    1e-10 (1 + max |A|) or ten times the estimate); without the quirk the T column of the path rows is zero, with it the documented formula;
    the arrow of H before the shift = differences of grad (lam_eq' c_eq) = A_eq' lam_eq, its diagonal after the shift the Gershgorin rule"""
    x0, xf, w, _ = _problems(narm, nseg)[0]
    P = R.Problem(_cfg(nseg, quirk_dtau_dT=0), _models(narm), x0, xf, LD)
    z = P.pack(*w)
    rng = np.random.default_rng(5)
    z = z + LD(1e-2) * rng.uniform(-1, 1, P.n)                   # (off the start guess: nothing pinned, no symmetric special point)
    lam = rng.uniform(-2, 2, P.m + P.n).astype(LD)
    Q = P.qp(z, lam)
    cols = np.arange(P.n) if at is None else np.concatenate([np.concatenate([P.ix(k), P.iu(k)]) for k in at] + [[P.iT]])
    A = Q["A"]
    bar = 1e-10 * (1 + float(np.abs(A).max()))
    for name, F, rows in (("dynamics", P.defects, slice(0, P.meq)), ("path", P.path_values, slice(P.meq, P.m))):
        J, est = _richardson(F, z, cols, 2.0 ** -17)
        d = np.abs(A[rows][:, cols] - J).astype(np.float64)
        assert np.all(d <= np.maximum(bar, 10 * est)), (name, d.max(), bar, est.max())
        assert np.abs(J).max() > 1                              # (the block is not empty)
    assert np.all(A[P.meq:, P.iT] == 0)
    assert np.all(Q["l"][:P.meq] == -P.defects(z)) and np.all(Q["u"][:P.meq] == Q["l"][:P.meq])
    # the quirk: d tau_i / dT := sum_j dv_ij qd_j + sum_{j >= i} M_ij qdd_j (rbd_reference.Reference.constraints); nothing else moves
    Pq = R.Problem(_cfg(nseg, quirk_dtau_dT=1), _models(narm), x0, xf, LD)
    Aq = Pq.qp(z, lam)["A"]
    keep = np.ones(P.n, dtype=bool); keep[P.iT] = False
    assert np.array_equal(Aq[:, keep], A[:, keep]) and np.array_equal(Aq[:P.meq], A[:P.meq])
    X, U, _ = P.unpack(z)
    for a, ref in enumerate(P.arms):
        xa, ua = P._arm(X, U, a)
        for k in range(P.N):
            col = ref.dtau_dqd(xa[k, :7], xa[k, 7:]) @ xa[k, 7:] + np.triu(ref.mass_matrix(xa[k, :7])) @ ua[k]
            rows = P.meq + P.ng * k + 7 * a + np.arange(7)
            assert np.abs(Aq[rows, P.iT] - col).max() < 1e-15 * (1 + np.abs(col).max())
            assert Aq[P.meq + P.ng * k + P.nq + a, P.iT] == 0
    assert np.abs(Aq[P.meq:, P.iT]).max() > 1e-2
    # Hessian arrow: grad_z (lam_eq' c_eq) = A_eq(z)' lam_eq is linear in z (c_eq is bilinear), so its central difference is exact to rounding
    grad = lambda Z: np.stack([P.dynamics_jacobian(zz).T @ lam[:P.meq] for zz in Z])
    Hd, _ = _richardson(grad, z, cols, 2.0 ** -4)
    assert np.abs(Hd - Q["H0"][:, cols]).max() < 1e-15 and np.abs(Q["H0"][:, cols]).max() > 1e-2
    H0, H = Q["H0"], Q["H"]
    off = ~np.eye(P.n, dtype=bool)
    assert np.array_equal(H[off], H0[off]) and np.all(np.diag(H0) == 0)
    r = np.abs(H0).sum(axis=1)
    assert np.abs(np.diag(H) - (r + LD(P.cfg.hess_reg))).max() < 1e-18 and np.count_nonzero(r) == P.nx * (P.N - 1) + 1
    # rho: the pinned start state and the dynamics rows take rho * rho_eq_scale, everything else rho
    eq = np.zeros(P.m + P.n, dtype=bool); eq[:P.meq] = True; eq[P.m + P.ix(0)] = True
    assert np.all(Q["rho"][eq] == LD(P.cfg.rho) * LD(P.cfg.rho_eq_scale)) and np.all(Q["rho"][~eq] == LD(P.cfg.rho))


# ---- the rounding floor ----------------------------------------------------------------------------------------------------------------------
def test_reference_rounding_floor():
    """float64 against long double at num_seg 1, 2, 4: the figures recorded in ocp_reference are what is measured here, and the bars (100 times
    them) are at most a tenth of the bars between kernels and oracle"""
    fp = fy = fx = fu = fT = 0.0
    for nseg in (1, 2, 4):
        for b in range(len(_problems(1, nseg))):
            for case in [c[0] for c in QP_CASES] + ["lin_warm"]:
                a, r = _ref_qp(1, nseg, b, case, np.float64), _ref_qp(1, nseg, b, case, LD)
                assert a[3] == r[3] and a[4] == r[4], (nseg, b, case)
                fp, fy = max(fp, _rel(a[1], r[1])), max(fy, _rel(a[2], r[2]))
            a, r = _ref_sqp(1, nseg, b, np.float64), _ref_sqp(1, nseg, b, LD)
            assert a[3]["qp_iters_total"] == r[3]["qp_iters_total"] and a[3]["last_alpha"] == r[3]["last_alpha"]
            fx, fu, fT = max(fx, _abs(a[0], r[0])), max(fu, _abs(a[1], r[1])), max(fT, abs(float(a[2] - r[2])) / float(r[2]))
    print("rounding floor: p %.2e  y %.2e  x %.2e  u %.2e  T %.2e" % (fp, fy, fx, fu, fT))
    # the recorded figures are such measurements, rounded up; another BLAS or thread count may round a little differently
    for got, rec in ((fp, R.FLOOR_P), (fy, R.FLOOR_Y), (fx, R.FLOOR_X), (fu, R.FLOOR_U), (fT, R.FLOOR_T)):
        assert got <= 3 * rec, (fp, fy, fx, fu, fT)
    assert R.P_BAR <= 1e-8 and R.Y_BAR <= 1e-7 and R.X_BAR <= 1e-7 and R.U_BAR <= 1e-6 and R.T_BAR <= 1e-7


# ---- the oracle's QP against the dense ADMM, and the certificate ------------------------------------------------------------------------------
def _odebug_qp(narm, cfg, x0, xf, pt, lam):
    lam = None if lam is None else np.asarray(lam, dtype=np.float64)
    return o.debug_qp(cfg, x0, xf, *pt, lam=lam) if narm == 1 else o.debug_qp_multi(_models(narm), cfg, x0, xf, *pt, lam=lam)


@pytest.mark.parametrize("narm,nseg", sorted(OFFSETS))
def test_oracle_qp_vs_dense_admm(narm, nseg):
    """orc_debug_qp / orc_debug_qp_multi against admm() (long double up to num_seg 4, float64 above) at the start guess (capped) and at the
    8-iteration point (convergent); one arm also both with the cap at 3 iterations and a test every iteration, and once with warm duals: equal
    iteration counts, p and y within the bars.  The certificate passes on the oracle's and on the reference's own (p, y) of every convergent QP,
    with at least one active inequality row each (so that its sign check says something), and its ratios fail on every capped one; over the
    cases both sides of the sign check are met; no termination test is a near tie"""
    real = _real(nseg)
    own, orc = 0.0, 0.0
    margin, dp, dy, upper, lower = np.inf, 0.0, 0.0, 0, 0
    for b, (x0, xf, w, lin) in enumerate(_problems(narm, nseg)):
        cases = [c[0] for c in QP_CASES] + (["lin_warm"] if b == 0 else []) if narm == 1 else ["start", "lin"]
        for case in cases:
            Q, p, y, its, capped, trace, cfg, pt, lam = _ref_qp(narm, nseg, b, case, real)
            what = (narm, nseg, b, case)
            margin = min(margin, R.termination_margin(trace))
            assert R.termination_margin(trace) >= TERMINATION_MARGIN, (what, "a termination test is a near tie: take another stream offset")
            assert len(trace) == its // cfg.check_every
            po, yo, ito = _odebug_qp(narm, cfg, x0, xf, pt, lam)
            assert ito == its, (what, ito, its)
            if narm == 1:       # (two arms start from the jerk-limited guess, whose QP may converge: there `capped` decides what is asked)
                assert capped == (case != "lin" and case != "lin_warm"), (what, its)
            assert capped == (its == cfg.qp_iters and max(trace[-1][1:]) > 1), (what, its, trace[-1])
            dp, dy = max(dp, _rel(po, p)), max(dy, _rel(yo, y))
            assert _rel(po, p) <= R.P_BAR, (what, _rel(po, p))
            assert _rel(yo, y) <= R.Y_BAR, (what, _rel(yo, y))
            cert, cert_own = R.certificate(cfg, Q, po, yo), R.certificate(cfg, Q, p, y)
            if capped:
                assert R.certificate_worst(cert) > 1 + 1e-6 and R.certificate_worst(cert_own) > 1 + 1e-6, (what, cert, cert_own)
            else:
                assert cert["active_upper"] + cert["active_lower"] >= 1 and cert_own["active_upper"] + cert_own["active_lower"] >= 1, (what, cert, cert_own)
                assert R.certificate_ok(cert) and R.certificate_ok(cert_own), (what, cert, cert_own)
                assert (cert["active_upper"], cert["active_lower"]) == (cert_own["active_upper"], cert_own["active_lower"]), (what, cert, cert_own)
                own, orc = max(own, R.certificate_worst(cert_own)), max(orc, R.certificate_worst(cert))
                upper, lower = upper + cert["active_upper"], lower + cert["active_lower"]
    assert upper >= 1 and lower >= 1, (narm, nseg, upper, lower)
    print("arms %d num_seg %d: largest certificate ratio %.3f (reference's own p, y), %.3f (oracle's); active inequality rows %d upper %d lower; "
          "closest termination test %.2e; oracle - reference p %.1e y %.1e" % (narm, nseg, own, orc, upper, lower, margin, dp, dy))


def test_certificate_rejects_a_wrong_dual_sign_and_a_shifted_step():
    """the certificate is not vacuous in its parts: the box duals negated fail the sign check (and stationarity), a step moved along a bounded
    direction fails the primal distance"""
    Q, p, y, its, capped, trace, cfg, pt, lam = _ref_qp(1, 1, 0, "lin", LD)
    assert R.certificate_ok(R.certificate(cfg, Q, p, y))
    m = Q["m"]
    yn = y.copy(); yn[m:] = -yn[m:]
    c = R.certificate(cfg, Q, p, yn)
    assert c["sign"] > 1 + 1e-6 and c["stationarity"] > 1 + 1e-6
    yn = -y
    assert R.certificate(cfg, Q, p, yn)["sign"] > 1 + 1e-6
    ps = p.copy(); ps[:14] += 0.05                     # (x_0 is pinned)
    assert R.certificate(cfg, Q, ps, y)["primal"] > 1 + 1e-6


# ---- the oracle's SQP against sqp() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm,nseg", sorted(OFFSETS))
def test_oracle_sqp_vs_reference(narm, nseg):
    """3 SQP iterations from the start guess: xs, us, T within the bars; last_alpha, qp_iters_total, qp_capped, sqp_iters and status equal; the four
    violation fields within the bars record_bars derives from the iterate's; no Armijo test and no termination test is a near tie"""
    real = _real(nseg)
    slack, margin, dx, du = np.inf, np.inf, 0.0, 0.0
    for b, (x0, xf, w, _) in enumerate(_problems(narm, nseg)):
        X, U, T, info, dg = _ref_sqp(narm, nseg, b, real)
        what = (narm, nseg, b)
        assert len(dg["traces"]) == 3 and len(dg["armijo"]) >= 3
        margin = min([margin] + [R.termination_margin(t) for t in dg["traces"]])
        slack = min([slack] + [abs(s) for s, _ in dg["armijo"]])
        assert min(R.termination_margin(t) for t in dg["traces"]) >= TERMINATION_MARGIN, (what, "near tie: take another stream offset")
        assert min(abs(s) for s, _ in dg["armijo"]) >= ARMIJO_MARGIN, (what, "an Armijo test is a near tie: take another stream offset")
        cfg = _cfg(nseg, 3)
        xs, us, To, oi = _osolve(narm, cfg, x0, xf, w)
        for k in ("last_alpha", "qp_iters_total", "qp_capped", "sqp_iters", "status"):
            assert getattr(oi, k) == info[k], (what, k, getattr(oi, k), info[k])
        dx, du = max(dx, _abs(xs, X)), max(du, _abs(us, U))
        assert _abs(xs, X) <= R.X_BAR and _abs(us, U) <= R.U_BAR and abs(To - float(T)) <= R.T_BAR * float(T), (what, _abs(xs, X), _abs(us, U), To - float(T))
        assert oi.T == To
        bars = R.record_bars(R.Problem(cfg, _models(narm), x0, xf, real), X, U, T, R.X_BAR, R.U_BAR, R.T_BAR * float(T))
        for k in ("viol_l1", "defect_inf", "path_viol_inf", "term_err_inf"):
            assert abs(getattr(oi, k) - info[k]) <= bars[k], (what, k, getattr(oi, k), info[k], bars[k])
        assert info["viol_l1"] > 0 and info["defect_inf"] > 0 and info["term_err_inf"] > 0
    print("arms %d num_seg %d: smallest Armijo slack %.2e, closest termination test %.2e, oracle - reference x %.1e u %.1e" % (narm, nseg, slack, margin, dx, du))


def test_sqp_honours_warm_duals_and_backtracks():
    """qp_warm_start = 1 and a final time fixed at 1 s (the searches backtrack, test_gpu_solver_settings.LS_FIXED_T): the oracle and sqp() agree on
    the step length, the iteration totals and the iterate there too, and both differ from the cold, free-T answer"""
    x0, xf, w, _ = _problems(1, 1)[0]
    cfg = _cfg(1, 3, qp_warm_start=1, lbT=1.0, ubT=1.0, ls_iters=5)
    X, U, T, info, dg = R.sqp(cfg, None, x0, xf, w, real=LD)
    assert min(abs(s) for s, _ in dg["armijo"]) >= ARMIJO_MARGIN and min(R.termination_margin(t) for t in dg["traces"]) >= TERMINATION_MARGIN
    assert any(not ok for _, ok in dg["armijo"]) and info["last_alpha"] < 1
    xs, us, To, oi = o.solve(cfg, x0, xf, *w)
    for k in ("last_alpha", "qp_iters_total", "qp_capped", "sqp_iters", "status"):
        assert getattr(oi, k) == info[k], (k, getattr(oi, k), info[k])
    assert _abs(xs, X) <= R.X_BAR and _abs(us, U) <= R.U_BAR and abs(To - float(T)) <= R.T_BAR * float(T)
    cold = o.Config.from_buffer_copy(bytes(cfg)); cold.qp_warm_start = 0
    assert np.abs(o.solve(cold, x0, xf, *w)[0] - xs).max() > 1e-6
