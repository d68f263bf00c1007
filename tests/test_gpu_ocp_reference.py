"""Every QP kernel path against the dense reference of the OCP / QP / SQP layer (tests/ocp_reference.py), which shares nothing with the oracle:
no sparse rows, no chain ordering, no skyline factor, and rigid-body terms from tests/rbd_reference.py.

  - one arm: Solver.qp at the convergent linearisation point and at the start guess, and both again with the cap at 3 iterations and a test every
    iteration, against the dense ADMM with the bars of test_gpu_solver_settings._check_qp; the epsilon-KKT certificate on the kernel's own (p, y);
  - two arms: a one-iteration solve from the linearisation point against sqp(), with the bars and fields of _check_solve;
  - every path: 3 SQP iterations from the start guess against sqp() the same way, and the violation fields of the result record.
Paths, contexts and problems are those of tests/test_gpu_solver_settings.py, the first two problems of each.  The reference runs on the host, in
long double up to num_seg 4 and in float64 above, once per discretisation.  Run with -m gpu."""
import types

import numpy as np
import pytest

import ocp_reference as R
import test_gpu_solver_settings as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


NB = 2                                   # problems per path
SHORT = dict(qp_iters=3, check_every=1)
QP_CASES = {"lin": ("lin", None), "start": ("start", None), "lin_short": ("lin", SHORT), "start_short": ("start", SHORT)}
ONE_ARM = [p[0] for p in S.PATHS if p[2] == 1]
TWO_ARM = [p[0] for p in S.PATHS if p[2] == 2]
TERMINATION_MARGIN, ARMIJO_MARGIN = 1e-6, 1e-9          # (as tests/test_ocp_reference_host.py)

_REF = {}


def _real(nseg):
    return np.longdouble if nseg <= 4 else np.float64


def _models(M, narm):
    return M.arm_models(M.DUAL_BASES) if narm == 2 else M.default_model()


def _points(narm, nseg, where):
    x0, xf, warm, lin = S._problems(narm, nseg, False)
    pt = lin if where == "lin" else warm
    return x0[:NB], xf[:NB], tuple(a[:NB] for a in pt)


def _ref_qp(M, nseg, case):
    """[(Q, p, y, iterations, capped, trace)] of the reference for the case's QPs, one per problem"""
    key = ("qp", nseg, case)
    if key not in _REF:
        where, fields = QP_CASES[case]
        cfg = S._config(nseg, 1, 1, fields)
        x0, xf, pt = _points(1, nseg, where)
        out = []
        for b in range(len(x0)):
            P = R.Problem(cfg, _models(M, 1), x0[b], xf[b], _real(nseg))
            Q = P.qp(P.pack(pt[0][b], pt[1][b], pt[2][b]))
            out.append((Q,) + R.admm(cfg, Q))
        _REF[key] = out
    return _REF[key]


def _ref_sqp(M, narm, nseg, iters, where):
    """[(xs, us, T, record, info dict, diagnostics)] of `iters` reference SQP iterations from the start guess / the linearisation point"""
    key = ("sqp", narm, nseg, iters, where)
    if key not in _REF:
        cfg = S._config(nseg, narm, iters, None)
        x0, xf, pt = _points(narm, nseg, where)
        out = []
        for b in range(len(x0)):
            X, U, T, info, dg = R.sqp(cfg, _models(M, narm), x0[b], xf[b], (pt[0][b], pt[1][b], pt[2][b]), real=_real(nseg))
            assert min(R.termination_margin(t) for t in dg["traces"]) >= TERMINATION_MARGIN, (narm, nseg, b, "a termination test is a near tie")
            assert min(abs(s) for s, _ in dg["armijo"]) >= ARMIJO_MARGIN, (narm, nseg, b, "an Armijo test is a near tie")
            out.append((X.astype(np.float64), U.astype(np.float64), float(T), types.SimpleNamespace(**info), info, dg))
        _REF[key] = out
    return _REF[key]


def _with_config(M, s, cfg, nseg, run):
    s.set_config(cfg)
    try:
        return run()
    finally:
        s.set_config(M.default_config(nseg, 1, margins=S.MARGINS))


@pytest.mark.parametrize("case", list(QP_CASES))
@pytest.mark.parametrize("path", ONE_ARM)
def test_qp_vs_dense_reference(M, path, case):
    """identical ADMM iteration counts, p <= 1e-7 (1 + |p|), y <= 1e-6 (1 + |y|) against the dense ADMM; where the QP converged the kernel's own
    (p, y) passes the certificate with at least one active inequality row, where it stopped at its cap the certificate's ratios fail (it is
    not vacuous)"""
    _, nseg, _, _, kname = S.PATH[path]
    where, fields = QP_CASES[case]
    ref = _ref_qp(M, nseg, case)
    for b, r in enumerate(ref):
        assert R.termination_margin(r[5]) >= TERMINATION_MARGIN, (path, case, b, "a termination test is a near tie")
        assert r[4] == (case != "lin"), (path, case, b, r[3])
    x0, xf, pt = _points(1, nseg, where)
    s = S._ctx(M, path)
    cfg = S._config(nseg, 1, 1, fields)
    p, y, it = _with_config(M, s, cfg, nseg, lambda: s.qp(x0, xf, *pt))
    assert s.kernel_timing()[0] == kname
    S._check_qp(1, (p, y, it), [(r[1].astype(np.float64), r[2].astype(np.float64), r[3]) for r in ref], (path, case))
    for b, r in enumerate(ref):
        cert = R.certificate(cfg, r[0], p[b], y[b])
        if case == "lin":               # (at least one inequality row carries a dual, or the sign check would say nothing)
            assert cert["active_upper"] + cert["active_lower"] >= 1, (path, case, b, cert)
            assert R.certificate_ok(cert), (path, case, b, cert)
        else:
            assert R.certificate_worst(cert) > 1 + 1e-6, (path, case, b, cert)


def _check_record(M, narm, nseg, got, ref, what):
    """viol_l1, defect_inf, path_viol_inf, term_err_inf of the kernel's record against the reference's.  The iterates may differ by the
    tolerances of _check_solve (1e-6 in x, 1e-5 in u, 1e-6 T in T); ocp_reference.record_bars turns those into bars of the fields: every constraint
    row moves by at most its Jacobian row's absolute sum weighted with them (doubled for the curvature), a maximum moves no more than its largest
    term, and the l1 sum by the sum over all rows plus one tolerance per box (the row count times the state tolerance, sharpened by the
    Jacobian).  Nothing here is fitted to what the kernels return."""
    sx, su, sT, info = got
    for b, (X, U, T, _, rec, _) in enumerate(ref):
        x0, xf, _ = _points(narm, nseg, "start")
        P = R.Problem(S._config(nseg, narm, 3, None), _models(M, narm), x0[b], xf[b], np.float64)
        bars = R.record_bars(P, X, U, T, 1e-6, 1e-5, 1e-6 * abs(T))
        for k in ("viol_l1", "defect_inf", "path_viol_inf", "term_err_inf"):
            assert abs(info[k][b] - rec[k]) <= bars[k], (what, b, k, info[k][b], rec[k], bars[k])
        assert info["sqp_iters"][b] == rec["sqp_iters"] and info["T"][b] == sT[b]


@pytest.mark.parametrize("path", TWO_ARM)
def test_two_arm_step_vs_reference(M, path):
    """two arms have no QP entry point: one SQP iteration from the linearisation point against sqp(): status, iteration totals, capped QPs,
    |dT| <= 1e-6 T, x <= 1e-6, u <= 1e-5"""
    _, nseg, narm, _, kname = S.PATH[path]
    ref = _ref_sqp(M, narm, nseg, 1, "lin")
    x0, xf, pt = _points(narm, nseg, "lin")
    s = S._ctx(M, path)
    got = _with_config(M, s, S._config(nseg, narm, 1, None), nseg, lambda: s.solve(x0, xf, pt))
    assert s.kernel_timing()[0] == kname
    S._check_solve(got, [r[:4] for r in ref], (path, "step"), alpha=False)


@pytest.mark.parametrize("path", [p[0] for p in S.PATHS])
def test_solve_vs_reference(M, path):
    """3 SQP iterations from the start guess against sqp(): status, iteration totals, capped QPs and last step length equal, |dT| <= 1e-6 T,
    x <= 1e-6, u <= 1e-5 (_check_solve), and the four violation fields of the record (_check_record)"""
    _, nseg, narm, _, kname = S.PATH[path]
    ref = _ref_sqp(M, narm, nseg, 3, "start")
    x0, xf, pt = _points(narm, nseg, "start")
    s = S._ctx(M, path)
    got = _with_config(M, s, S._config(nseg, narm, 3, None), nseg, lambda: s.solve(x0, xf, pt))
    assert s.kernel_timing()[0] == kname
    S._check_solve(got, [r[:4] for r in ref], (path, "solve"))
    _check_record(M, narm, nseg, got, ref, path)
