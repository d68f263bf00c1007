"""The optimal-control problem, its QP and the SQP iteration as dense linear algebra (plain numpy): a reference for the layer above the rigid body.

The oracle (oracle/ocp.c) and the kernels assemble sparse rows, order the variables along the chain and factorise a skyline / block matrix.  This
module does none of that.  It is written from the specification alone (include/mpcmp.h: variable layout, row order, mpcmp_config, mpcmp_info and
the status bits) and keeps every matrix dense:

    z = [x_0 .. x_{N-1} | u_0 .. u_{N-1} | T],  N = 3 num_seg + 1,  x_k = [q(7 narm); qd(7 narm)],  u_k = qdd(7 narm),  n = 21 narm N + 1
    rows: dynamics (14 narm per node, nodes 0 .. N-2), then path (8 narm per node: [tau(7 narm); z_tool(narm)]), then the n boxes
    dynamics of segment s, local node i in {0, 1, 2}, k = 3 s + i:   sum_j D[i][j] x_{3s+j} - ts T [qd_k; u_k] = 0,   ts = 1 / (2 num_seg)

  - the differentiation matrix comes from the node positions by the barycentric form of Lagrange differentiation;
  - path values and their Jacobians come from tests/rbd_reference.py (energies and Lagrange's equations, no Newton-Euler recursion);
  - the QP min 1/2 p'Hp + e_T'p, l <= [A; I] p <= u is solved by the OSQP-form ADMM with the reduced matrix
    K = H + sigma I + [A; I]' diag(rho) [A; I], inverted once by a hand-written Cholesky (numpy.linalg has no long double).  The inverse is kept
    as the explicit inverse factor, K^-1 b = L^-T (L^-1 b): the product L^-T L^-1 formed once loses cond(K) (1e6 here) in float64 and made the
    float64 run a hundred times noisier than the oracle's skyline solve; the factored form is as accurate as substitution;
  - certificate(): what a returned (p, y) must satisfy when the ADMM stopped below its cap, with bounds that follow from mpcmp_config alone;
  - sqp(): the l1-merit line search, multiplier update and relinearisation, and the result record of mpcmp_info.

`real` is np.float64 or np.longdouble.  Everything here is for tests; nothing is fast.

Measured accuracy (tests/test_ocp_reference_host.py::test_reference_rounding_floor, x86-64 80-bit long double, one arm, num_seg 1, 2, 4: per problem
the QPs at the start guess (capped at 700 iterations) and at the 8-iteration point (convergent), both again capped at 3 iterations, one with warm
duals, and 3 SQP iterations from the start guess).  Float64 against long double, this module against itself, largest difference:

    p  7.5e-12 (1 + |p|_inf), |p| up to 6.5       y  1.6e-12 (1 + |y|_inf)       after 3 SQP iterations  x 1.1e-10,  u 4.2e-10,  T 6.5e-12 T

That is the rounding floor of a dense float64 solve of these QPs (FLOOR_*).  The bars of the oracle against this module are 100 times the floor (the
skyline Cholesky and the dense inverse factor round differently over up to 700 dependent iterations, and three SQP iterations build on each
other): P_BAR 7.5e-10, Y_BAR 1.6e-10 (times 1 + the largest entry), X_BAR 1.1e-8, U_BAR 4.2e-8, T_BAR 6.5e-10 (relative).  Each is a tenth or
less of the bar between kernels and oracle (1e-7 (1 + |p|), 1e-6 (1 + |y|), 1e-6 in x, 1e-5 in u, 1e-6 T), which the same test asserts.
Measured, oracle against this module in long double: p 2e-11, x 1.4e-10, u 5e-10.

The rounding threshold of the certificate for an inactive dual that is not exactly zero is 1e-9 (1 + |y|_inf): an inactive row's update
y + rho (z_relaxed - clip(z_relaxed + y / rho)) cancels to a few units in the last place of y, seven orders below that.

The status bit MPCMP_STATUS_T_OUT_OF_BOX is taken as include/mpcmp.h words it: T < lbT or T > ubT, without a rounding allowance.
"""
import numpy as np

import rbd_reference as rbd

# measured by test_reference_rounding_floor (see the docstring); the bars follow from them
FLOOR_P, FLOOR_Y, FLOOR_X, FLOOR_U, FLOOR_T = 7.5e-12, 1.6e-12, 1.1e-10, 4.2e-10, 6.5e-12
P_BAR, Y_BAR, X_BAR, U_BAR, T_BAR = 100 * FLOOR_P, 100 * FLOOR_Y, 100 * FLOOR_X, 100 * FLOOR_U, 100 * FLOOR_T

STATUS_NAN, STATUS_NOT_PD, STATUS_QP_CAPPED, STATUS_OUTSIDE_TOL, STATUS_T_OUT_OF_BOX = 1, 2, 8, 16, 32      # include/mpcmp.h
RHO_EQ_WIDTH = 1e-4          # a row or box narrower than this takes rho * rho_eq_scale (include/mpcmp.h)
INFO_FIELDS = ("T", "viol_l1", "defect_inf", "path_viol_inf", "term_err_inf", "last_alpha", "qp_iters_total", "sqp_iters", "status", "qp_capped")


# ---- grid ------------------------------------------------------------------------------------------------------------------------------------
def local_nodes(real=np.float64):
    """cubic Chebyshev-Gauss-Lobatto points -cos(j pi / 3), j = 0 .. 3, on [-1, 1]: -1, -1/2, 1/2, 1 (cos(pi / 3) = 1/2 exactly)"""
    xi = np.array([-1, -0.5, 0.5, 1], dtype=real)
    assert np.abs(xi + np.cos(np.pi * np.arange(4) / 3)).max() < 1e-15
    return xi


def nodes(num_seg, real=np.float64):
    """the N = 3 num_seg + 1 ascending node times on [0, 1]: num_seg equal segments, neighbours share their end node"""
    xi = local_nodes(real)
    t = [(s + (xi[j] + 1) / 2) / real(num_seg) for s in range(num_seg) for j in range(3)]
    return np.array(t + [real(1)], dtype=real)


def diff_matrix(real=np.float64):
    """D[i][j] = l_j'(xi_i) of the Lagrange basis on the local nodes, in the barycentric form: w_j = 1 / prod_{k != j} (xi_j - xi_k),
    D_ij = (w_j / w_i) / (xi_i - xi_j) off the diagonal, D_ii = - sum_{j != i} D_ij (the derivative of a constant is zero)"""
    xi = local_nodes(real)
    d = xi[:, None] - xi[None, :] + np.eye(4, dtype=real)
    w = 1 / d.prod(axis=1)
    D = (w[None, :] / w[:, None]) / d
    D[np.arange(4), np.arange(4)] = 0
    D[np.arange(4), np.arange(4)] = -D.sum(axis=1)
    return D


def _models(models):
    """None (the compiled-in Panda of the oracle), a ctypes Model, or a sequence of them: a list of rbd_reference field dicts, one per arm"""
    if models is None:
        import oracle_py
        models = [oracle_py.default_model()]
    if hasattr(models, "R0"):
        models = [models]
    return [m if isinstance(m, dict) else rbd.model_fields(m) for m in models]


class Problem:
    """one OCP: configuration (any object with the fields of mpcmp_config), arm models, start and target state, precision"""

    def __init__(self, cfg, models, x0, xf, real=np.float64):
        self.cfg, self.real = cfg, real
        self.arms = [rbd.Reference(real=real, **m) for m in _models(models)]
        self.narm = narm = len(self.arms)
        self.N = N = 3 * cfg.num_seg + 1
        self.nq, self.nx, self.nu, self.ng = 7 * narm, 14 * narm, 7 * narm, 8 * narm
        self.n = (self.nx + self.nu) * N + 1
        self.meq, self.min = self.nx * (N - 1), self.ng * N
        self.m = self.meq + self.min
        self.ts = real(1) / real(2 * cfg.num_seg)
        self.D = diff_matrix(real)
        self.x0, self.xf = np.asarray(x0, dtype=real), np.asarray(xf, dtype=real)
        self.iT = self.n - 1
        self.zlb, self.zub = self.boxes()
        # bounds of the path rows of one node: torques of every arm, then the tool height of every arm
        self.lbg = np.array([cfg.lbg[j] for _ in range(narm) for j in range(7)] + [cfg.lbg[7]] * narm, dtype=real)
        self.ubg = np.array([cfg.ubg[j] for _ in range(narm) for j in range(7)] + [cfg.ubg[7]] * narm, dtype=real)

    # ---- layout ----
    def ix(self, k):
        return np.arange(self.nx * k, self.nx * (k + 1))

    def iu(self, k):
        return self.nx * self.N + np.arange(self.nu * k, self.nu * (k + 1))

    def pack(self, xs, us, T):
        return np.concatenate([np.asarray(xs, dtype=self.real).ravel(), np.asarray(us, dtype=self.real).ravel(), [self.real(T)]])

    def unpack(self, z):
        """X [..., N, nx], U [..., N, nu], T [...] of z [..., n]"""
        lead = z.shape[:-1]
        nX = self.nx * self.N
        return z[..., :nX].reshape(lead + (self.N, self.nx)), z[..., nX:self.n - 1].reshape(lead + (self.N, self.nu)), z[..., -1]

    def _arm(self, X, U, a):
        """[q_a; qd_a] [..., N, 14] and qdd_a [..., N, 7] of arm a"""
        nq = self.nq
        return np.concatenate([X[..., 7 * a:7 * a + 7], X[..., nq + 7 * a:nq + 7 * a + 7]], axis=-1), U[..., 7 * a:7 * a + 7]

    # ---- the NLP ----
    def boxes(self):
        """(lb, ub) [n] of the variables: x_0 pinned to the start, x_{N-1} within eps_target of the target, the other states, the controls and T
        within the tables of the configuration (every arm reads the same tables)"""
        c, real, N, narm = self.cfg, self.real, self.N, self.narm
        lbx = np.array([c.lbx[j] for _ in range(narm) for j in range(7)] + [c.lbx[7 + j] for _ in range(narm) for j in range(7)], dtype=real)
        ubx = np.array([c.ubx[j] for _ in range(narm) for j in range(7)] + [c.ubx[7 + j] for _ in range(narm) for j in range(7)], dtype=real)
        lb, ub = np.zeros(self.n, dtype=real), np.zeros(self.n, dtype=real)
        for k in range(N):
            lb[self.ix(k)], ub[self.ix(k)] = lbx, ubx
            lb[self.iu(k)] = np.array(list(c.lbu[:7]) * narm, dtype=real)
            ub[self.iu(k)] = np.array(list(c.ubu[:7]) * narm, dtype=real)
        lb[self.ix(0)] = ub[self.ix(0)] = self.x0
        lb[self.ix(N - 1)], ub[self.ix(N - 1)] = self.xf - real(c.eps_target), self.xf + real(c.eps_target)
        lb[self.iT], ub[self.iT] = real(c.lbT), real(c.ubT)
        return lb, ub

    def _rates(self, X, U):
        """f_k = [qd_k; u_k] [..., N, nx]"""
        return np.concatenate([X[..., self.nq:], U], axis=-1)

    def defects(self, z):
        """collocation defects [..., meq] at z [..., n]"""
        X, U, T = self.unpack(z)
        f = self._rates(X, U)
        out = []
        for s in range(self.cfg.num_seg):
            dX = np.einsum("ij,...jr->...ir", self.D[:3], X[..., 3 * s:3 * s + 4, :])
            out.append(dX - self.ts * T[..., None, None] * f[..., 3 * s:3 * s + 3, :])
        out = np.concatenate(out, axis=-2)
        return out.reshape(out.shape[:-2] + (self.meq,))

    def path_values(self, z):
        """path rows [..., min] at z [..., n]: per node the torques of every arm, then the tool height of every arm"""
        X, U, _ = self.unpack(z)
        tau, hgt = [], []
        for a, ref in enumerate(self.arms):
            xa, ua = self._arm(X, U, a)
            tau.append(ref.tau(xa[..., :7], xa[..., 7:], ua))
            hgt.append(ref.fk(xa[..., :7])["tool"][..., 2:3])
        g = np.concatenate(tau + hgt, axis=-1)
        return g.reshape(g.shape[:-2] + (self.min,))

    def dynamics_jacobian(self, z):
        """dense d defects / d z [meq, n]"""
        real, nq, nx = self.real, self.nq, self.nx
        X, U, T = self.unpack(z)
        f = self._rates(X, U)
        A = np.zeros((self.meq, self.n), dtype=real)
        I = np.eye(nx, dtype=real)
        for k in range(self.N - 1):
            s, i = divmod(k, 3)
            rows = np.arange(nx * k, nx * (k + 1))
            for j in range(4):
                A[np.ix_(rows, self.ix(3 * s + j))] += self.D[i, j] * I
            fcols = np.concatenate([self.ix(k)[nq:], self.iu(k)])
            A[rows, fcols] += -self.ts * T
            A[rows, self.iT] += -self.ts * f[k]
        return A

    def path_jacobian(self, z, quirk=None):
        """dense d path rows / d z [min, n] from rbd_reference.Reference.constraints (quirk: default the configuration's quirk_dtau_dT), and
        the values"""
        X, U, _ = self.unpack(z)
        G = np.zeros((self.min, self.n), dtype=self.real)
        g = np.zeros(self.min, dtype=self.real)
        for a, ref in enumerate(self.arms):
            xa, ua = self._arm(X, U, a)
            ga, Ga, _ = ref.constraints(xa, ua, quirk=self.cfg.quirk_dtau_dT if quirk is None else quirk)
            for k in range(self.N):
                rows = self.ng * k + np.array([7 * a + r for r in range(7)] + [self.nq + a])
                g[rows] = ga[k]
                G[np.ix_(rows, self.ix(k)[7 * a:7 * a + 7])] = Ga[k][:, 0:7]
                G[np.ix_(rows, self.ix(k)[self.nq + 7 * a:self.nq + 7 * a + 7])] = Ga[k][:, 7:14]
                G[np.ix_(rows, self.iu(k)[7 * a:7 * a + 7])] = Ga[k][:, 14:21]
                G[rows, self.iT] += Ga[k][:, 21]
        return G, g

    def hessian(self, z, lam):
        """(H, H0): H0 = the Hessian of lam_eq' c_eq, whose only entries are d2 / dT d f_k = -ts lam_k (an arrow on the T row and column: the
        path rows and the cost contribute nothing); H = H0 after the Gershgorin shift: every diagonal entry whose disc
        reaches zero or below, a_ii - r_i <= 0 with r_i = sum_{j != i} |a_ij|, is raised to r_i + hess_reg"""
        real, nq = self.real, self.nq
        H0 = np.zeros((self.n, self.n), dtype=real)
        lam_eq = np.asarray(lam, dtype=real)[:self.meq].reshape(self.N - 1, self.nx)
        for k in range(self.N - 1):
            fcols = np.concatenate([self.ix(k)[nq:], self.iu(k)])
            H0[fcols, self.iT] += -self.ts * lam_eq[k]
            H0[self.iT, fcols] += -self.ts * lam_eq[k]
        H = H0.copy()
        d = np.diag(H0)
        r = np.abs(H0).sum(axis=1) - np.abs(d)
        low = d - r <= 0
        H[np.arange(self.n)[low], np.arange(self.n)[low]] = (r + real(self.cfg.hess_reg))[low]
        return H, H0

    def qp(self, z, lam=None):
        """the QP of the step p at (z, lam): dict with A [m, n], l, u [m + n], H, H0 [n, n], q = e_T, rho [m + n], and the constraint values
        ceq [meq], g [min] it was linearised at"""
        c, real = self.cfg, self.real
        z = np.asarray(z, dtype=real)
        lam = np.zeros(self.m + self.n, dtype=real) if lam is None else np.asarray(lam, dtype=real)
        ceq = self.defects(z)
        Gp, g = self.path_jacobian(z)
        A = np.vstack([self.dynamics_jacobian(z), Gp])
        N = self.N
        l = np.concatenate([-ceq, np.tile(self.lbg, N) - g, self.zlb - z])
        u = np.concatenate([-ceq, np.tile(self.ubg, N) - g, self.zub - z])
        H, H0 = self.hessian(z, lam)
        q = np.zeros(self.n, dtype=real); q[self.iT] = 1
        rho = np.where(u - l < real(RHO_EQ_WIDTH), real(c.rho) * real(c.rho_eq_scale), real(c.rho)).astype(real)
        return dict(A=A, l=l, u=u, H=H, H0=H0, q=q, rho=rho, ceq=ceq, g=g, m=self.m, n=self.n)

    # ---- merit ----
    def violation(self, z, ceq=None, g=None):
        """dict: l1 (sum of |defects|, of the path rows' distance to [lbg, ubg] and of the variables' distance to their boxes), defect_inf,
        path_viol_inf"""
        ceq = self.defects(z) if ceq is None else ceq
        g = self.path_values(z) if g is None else g
        zero = self.real(0)
        vg = np.maximum(np.maximum(np.tile(self.lbg, self.N) - g, g - np.tile(self.ubg, self.N)), zero)
        vz = np.maximum(np.maximum(self.zlb - z, z - self.zub), zero)
        return dict(l1=np.abs(ceq).sum() + vg.sum() + vz.sum(), defect_inf=np.abs(ceq).max(), path_viol_inf=vg.max())


def record_bars(P, X, U, T, x_tol, u_tol, T_tol):
    """How far the violation fields of two result records may differ when their iterates differ by at most x_tol, u_tol, T_tol (absolute).
    Row i of the constraints moves by at most b_i = sum_j |dc_i / dz_j| tol_j to first order (the true Jacobian: no quirk column); the distance
    of a value to an interval, a maximum and a sum move no more than their arguments.  The bars are twice the first-order bounds: the second-order
    remainder is smaller than the first-order term by the factor tol |d2c| / |dc|, far below one at tolerances of 1e-5 and less.
        defect_inf 2 max b_i (dynamics)    path_viol_inf 2 max b_i (path)    term_err_inf x_tol    viol_l1 2 sum b_i + sum_j tol_j (the boxes)"""
    z = P.pack(X, U, T)
    A = np.abs(np.vstack([P.dynamics_jacobian(z), P.path_jacobian(z, quirk=0)[0]])).astype(np.float64)
    tol = np.concatenate([np.full(P.nx * P.N, x_tol), np.full(P.nu * P.N, u_tol), [T_tol]]).astype(np.float64)
    b = A @ tol
    return dict(defect_inf=2 * b[:P.meq].max(), path_viol_inf=2 * b[P.meq:].max(), term_err_inf=float(x_tol), viol_l1=2 * b.sum() + tol.sum())


# ---- linear algebra ---------------------------------------------------------------------------------------------------------------------------
def cholesky_inverse(K):
    """K^-1 of a symmetric positive definite K in K's own dtype: K = L L', K^-1 = L^-T L^-1.  Raises ArithmeticError when a pivot is not positive"""
    n = K.shape[0]
    L = np.tril(K).copy()
    for j in range(n):
        d = L[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise ArithmeticError("pivot %d is not positive" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros_like(L)
    for i in range(n):
        e = np.zeros(n, dtype=K.dtype); e[i] = 1
        Li[i] = (e - L[i, :i] @ Li[:i]) / L[i, i]
    return Li


def _inf(v):
    return np.abs(v).max()


def admm(cfg, qp, y0=None):
    """OSQP-form ADMM on l <= [A; I] p <= u with per-row rho and relaxation alpha.  Start x = 0, y = 0, z = 0; with y0 (the warm
    start of qp_warm_start): y = y0, z = clip(0, l, u).  Every check_every iterations it stops when
    |[A; I] x - z|_inf <= eps_abs + eps_rel max(|[A; I] x|, |z|) and |Hx + q + [A; I]' y|_inf <= eps_abs + eps_rel max(|Hx|, |[A; I]' y|, |q| = 1).
    Returns p, y, iterations, capped, trace: trace holds (iteration, primal residual / threshold, dual residual / threshold) of every test"""
    A, l, u, H, q, rho = (qp[k] for k in ("A", "l", "u", "H", "q", "rho"))
    real = A.dtype.type
    n = A.shape[1]
    AI = np.vstack([A, np.eye(n, dtype=real)])
    AIt = np.ascontiguousarray(AI.T)
    sigma, alpha = real(cfg.sigma), real(cfg.alpha)
    Li = cholesky_inverse(H + sigma * np.eye(n, dtype=real) + AIt @ (rho[:, None] * AI))
    Lit = np.ascontiguousarray(Li.T)
    x = np.zeros(n, dtype=real); y = np.zeros(AI.shape[0], dtype=real); z = np.zeros(AI.shape[0], dtype=real)
    if y0 is not None:
        y = np.asarray(y0, dtype=real).copy()
        z = np.clip(z, l, u)
    eps_abs, eps_rel = real(cfg.eps_abs), real(cfg.eps_rel)
    trace, capped, it = [], True, 0
    for it in range(1, cfg.qp_iters + 1):
        xt = Lit @ (Li @ (sigma * x - q + AIt @ (rho * z - y)))
        zt = AI @ xt
        x = alpha * xt + (1 - alpha) * x
        zr = alpha * zt + (1 - alpha) * z
        z = np.clip(zr + y / rho, l, u)
        y = y + rho * (zr - z)
        if it % cfg.check_every == 0:
            Ax, Hx, Aty = AI @ x, H @ x, AIt @ y
            rp, rd = _inf(Ax - z), _inf(Hx + q + Aty)
            ep = eps_abs + eps_rel * max(_inf(Ax), _inf(z))
            ed = eps_abs + eps_rel * max(_inf(Hx), _inf(Aty), real(1))
            trace.append((it, float(rp / ep) if ep > 0 else np.inf, float(rd / ed) if ed > 0 else np.inf))
            if rp <= ep and rd <= ed:
                capped = False
                break
    return x, y, it, capped, trace


def termination_margin(trace):
    """the smallest relative distance |ratio - 1| of a residual to its threshold over all tests of a trace (inf when there was no test)"""
    return min([min(abs(a - 1), abs(b - 1)) for _, a, b in trace], default=np.inf)


def certificate(cfg, qp, p, y, thr_scale=1e-9):
    """What (p, y) returned by an ADMM that met its termination test must satisfy.  With Abar = [A; I], r_p = |Abar p - z|_inf and z in [l, u]:
    the test gives r_p <= eps_abs + eps_rel max(|Abar p|, |z|) and |z| <= |Abar p| + r_p, hence r_p <= eps_p = (eps_abs + eps_rel |Abar p|) /
    (1 - eps_rel).  The dual update y <- rho (z_relaxed + y / rho - clip(..)) makes y_i > 0 only where z_i = u_i and y_i < 0 only where
    z_i = l_i.  So:
        stationarity     |Hp + q + Abar' y|_inf <= eps_abs + eps_rel max(|Hp|, |Abar' y|, 1)                      (the dual test itself)
        primal distance  dist_inf(Abar p, [l, u]) <= eps_p
        sign             y_i > thr: (Abar p)_i >= u_i - eps_p;     y_i < -thr: (Abar p)_i <= l_i + eps_p,    thr = 1e-9 (1 + |y|_inf)
    On an equality row (u_i - l_i < 1e-4: the dynamics rows, the pinned start state, a locked joint) the sign condition says no more than the
    primal distance, and such rows always carry a dual; so the rows that make the sign check say something are the inequality rows with a dual.
    Returns a dict of the three ratios to their bounds (sign: the larger of the two sides) and active_upper / active_lower: the number of
    inequality rows with y_i > thr / y_i < -thr.  certificate_ok: every ratio at most 1 + 1e-6 and at least one active inequality row"""
    A, l, u, H, q = (qp[k] for k in ("A", "l", "u", "H", "q"))
    real = A.dtype.type
    p, y = np.asarray(p, dtype=real), np.asarray(y, dtype=real)
    m = A.shape[0]
    Ap = np.concatenate([A @ p, p])
    Hp, Aty = H @ p, A.T @ y[:m] + y[m:]
    eps_abs, eps_rel = real(cfg.eps_abs), real(cfg.eps_rel)
    ed = eps_abs + eps_rel * max(_inf(Hp), _inf(Aty), real(1))
    ep = (eps_abs + eps_rel * _inf(Ap)) / (1 - eps_rel)
    dist = np.maximum(np.maximum(l - Ap, Ap - u), real(0)).max()
    thr = real(thr_scale) * (1 + _inf(y))
    pos, neg = y > thr, y < -thr
    gap = max((u - Ap)[pos].max() if pos.any() else real(0), (Ap - l)[neg].max() if neg.any() else real(0))
    ineq = u - l >= real(RHO_EQ_WIDTH)
    return dict(stationarity=float(_inf(Hp + q + Aty) / ed), primal=float(dist / ep), sign=float(gap / ep),
                active_upper=int((pos & ineq).sum()), active_lower=int((neg & ineq).sum()))


def certificate_worst(cert):
    """the largest of the three ratios"""
    return max(cert["stationarity"], cert["primal"], cert["sign"])


def certificate_ok(cert):
    return cert["active_upper"] + cert["active_lower"] > 0 and certificate_worst(cert) <= 1 + 1e-6


# ---- SQP ----------------------------------------------------------------------------------------------------------------------------------
def sqp(cfg, models, x0, xf, guess, lam0=None, real=np.float64):
    """cfg.sqp_iters iterations of the l1-merit line-search SQP from guess = (xs, us, T), multipliers lam0 (default 0):
        QP at (z, lam) -> (p, y), started from y = lam when cfg.qp_warm_start is set;
        mu = |lam|_inf, phi(z) = T + mu viol_l1(z), D phi = p_T - mu viol_l1(z);
        alpha = 1, multiplied by ls_tau at most ls_iters - 1 times while phi(z + alpha p) > phi(z) + alpha ls_eta D phi;
        z += alpha p, lam += alpha (y - lam), relinearise.
    Returns xs, us, T, info (dict with the fields of mpcmp_info), and a dict of diagnostics: armijo = (relative slack, accepted) of every Armijo
    test, slack = (bound - phi(z + alpha p)) / max(1, |phi(z)|, |phi(z + alpha p)|); traces = the ADMM trace of every QP; lam = the multipliers"""
    P = Problem(cfg, models, x0, xf, real)
    z = P.pack(*guess)
    lam = np.zeros(P.m + P.n, dtype=real) if lam0 is None else np.asarray(lam0, dtype=real).copy()
    info = dict.fromkeys(INFO_FIELDS, 0)
    armijo, traces = [], []
    for it in range(cfg.sqp_iters):
        Q = P.qp(z, lam)
        try:
            p, y, its, capped, trace = admm(cfg, Q, lam if cfg.qp_warm_start == 1 else None)
        except ArithmeticError:
            info["status"] |= STATUS_NOT_PD
            break
        traces.append(trace)
        info["qp_iters_total"] += its
        if capped:
            info["status"] |= STATUS_QP_CAPPED; info["qp_capped"] += 1
        mu = _inf(lam)
        viol = P.violation(z, Q["ceq"], Q["g"])["l1"]
        phi = z[-1] + mu * viol
        dphi = p[-1] - mu * viol
        alpha = real(1)
        for _ in range(1, cfg.ls_iters):
            zs = z + alpha * p
            phis = zs[-1] + mu * P.violation(zs)["l1"]
            bound = phi + alpha * real(cfg.ls_eta) * dphi
            ok = bool(phis <= bound)
            armijo.append((float((bound - phis) / max(real(1), abs(phi), abs(phis))), ok))
            if ok:
                break
            alpha = alpha * real(cfg.ls_tau)
        z = z + alpha * p
        lam = lam + alpha * (y - lam)
        info["last_alpha"] = float(alpha); info["sqp_iters"] = it + 1
    X, U, T = P.unpack(z)
    v = P.violation(z)
    info["T"] = float(T)
    info["viol_l1"], info["defect_inf"], info["path_viol_inf"] = float(v["l1"]), float(v["defect_inf"]), float(v["path_viol_inf"])
    info["term_err_inf"] = float(_inf(X[-1] - P.xf))
    if not np.all(np.isfinite(z)):
        info["status"] |= STATUS_NAN
    if info["defect_inf"] > cfg.eps_abs or info["path_viol_inf"] > cfg.eps_abs or info["term_err_inf"] > cfg.eps_target + cfg.eps_abs:
        info["status"] |= STATUS_OUTSIDE_TOL
    if not (cfg.lbT <= info["T"] <= cfg.ubT):
        info["status"] |= STATUS_T_OUT_OF_BOX
    return X.copy(), U.copy(), T, info, dict(armijo=armijo, traces=traces, lam=lam)
