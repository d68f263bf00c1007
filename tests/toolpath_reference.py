"""The rule of the tool-line moves (include/mpcmp_toolpath.h) restated in NumPy, independently of the library: its own forward kinematics from the
model's fields, its own Jacobian, logarithm, exponential, Cholesky-free solves (numpy.linalg), the closed-form derivative of the velocity field
from the partial derivatives of the Jacobian (dJ/dq_i, the O(n^2) form, not the recursion the library uses), the predictor / corrector
continuation with its stop rule, the nodes, and the deviation check.  Nothing here calls the library's kinematics."""
import numpy as np

STOPPED, Q_OUT_OF_BOUNDS, TD_OVER, NAN = 1, 2, 1, 128
DEFAULT_SPEC = dict(tool_lin_max=1.7, tool_ang_max=2.5, T_min=0.2, damp=1e-8, manip_min=1e-3, eps=1e-9, n_sub=4)


def model_arrays(model):
    """(R0 [7][3][3], p [7][3], tool [3]) of a ctypes Model"""
    return (np.array([list(model.R0[i]) for i in range(7)]).reshape(7, 3, 3), np.array([list(model.p[i]) for i in range(7)]),
            np.array(list(model.tool)))


def fk(m, q):
    """tool rotation, tool position, joint axes [7][3] and joint origins [7][3] in the world frame"""
    R0, pj, tool = m
    R, p = np.eye(3), np.zeros(3)
    z, o = np.zeros((7, 3)), np.zeros((7, 3))
    for i in range(7):
        p = p + R @ pj[i]
        c, s = np.cos(q[i]), np.sin(q[i])
        R = R @ R0[i] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        z[i], o[i] = R[:, 2], p
    return R, p + R @ tool, z, o


def jacobian(m, q):
    """world-aligned 6x7 Jacobian of the tool frame, rows [linear; angular], with the pose and the chain it was formed from"""
    R, p, z, o = fk(m, q)
    J = np.zeros((6, 7))
    for i in range(7):
        J[:3, i] = np.cross(z[i], p - o[i]); J[3:, i] = z[i]
    return J, R, p, z, o


def log3(R):
    """rotation vector of R"""
    ct = min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    th = np.arccos(ct)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-8:
        return 0.5 * v
    if np.pi - th > 1e-4:
        return th / (2.0 * np.sin(th)) * v
    a = np.sqrt(np.maximum(0.0, (np.diag(R) - ct) / (1.0 - ct)))
    return th * np.where(v < 0.0, -1.0, 1.0) * a


def exp3(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-4:
        return np.eye(3) + (1.0 - th * th / 6.0) * K + (0.5 - th * th / 24.0) * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * K @ K


def sigma(s):
    return 10.0 * s ** 3 - 15.0 * s ** 4 + 6.0 * s ** 5


def sigma1(s):
    return 30.0 * s ** 2 - 60.0 * s ** 3 + 30.0 * s ** 4


def sigma2(s):
    return 60.0 * s - 180.0 * s ** 2 + 120.0 * s ** 3


def time_nodes(nseg):
    xi = np.array([-1.0, -0.5, 0.5, 1.0])
    t = np.zeros(3 * nseg + 1)
    for s in range(nseg):
        t[3 * s:3 * s + 4] = (s + 0.5 * (xi + 1.0)) / nseg
    return t


def line(m, q_start, R1, p1):
    """(R0, p0, w, V) of the line from the tool pose at q_start to (R1, p1)"""
    R0, p0, _, _ = fk(m, q_start)
    w = log3(R0.T @ R1)
    return R0, p0, w, np.concatenate([p1 - p0, R0 @ w])


def field(m, q, V, damp):
    """g(q) = J^T (J J^T + damp I)^-1 V"""
    J = jacobian(m, q)[0]
    return J.T @ np.linalg.solve(J @ J.T + damp * np.eye(6), V)


def field_derivative(m, q, V, damp):
    """g' = the derivative of g along itself: J'^T y - J^T A^-1 (J' J^T y + J J'^T y) with J' = sum_i (dJ / dq_i) g_i.  For a revolute chain,
    with d_j = p - o_j:  d(z_j)/dq_i = z_i x z_j (i < j, else 0);  d(z_j x d_j)/dq_i = (z_i x z_j) x d_j + z_j x (z_i x d_j) for i < j and
    z_j x (z_i x d_i) for i >= j."""
    J, R, p, z, o = jacobian(m, q)
    A = J @ J.T + damp * np.eye(6)
    y = np.linalg.solve(A, V)
    g = J.T @ y
    Jp = np.zeros((6, 7))
    for i in range(7):
        dJ = np.zeros((6, 7))
        for j in range(7):
            if i < j:
                dz = np.cross(z[i], z[j])
                dJ[:3, j] = np.cross(dz, p - o[j]) + np.cross(z[j], np.cross(z[i], p - o[j]))
                dJ[3:, j] = dz
            else:
                dJ[:3, j] = np.cross(z[j], np.cross(z[i], p - o[i]))
        Jp += dJ * g[i]
    return Jp.T @ y - J.T @ np.linalg.solve(A, Jp @ g + J @ (Jp.T @ y)), g


def field_derivative_svd(m, q, V, damp):
    """(g', g) once more, with every (J J^T + damp I)^-1 applied through the singular value decomposition of J instead of a solve: the same
    quantities by another route, so that the difference from field_derivative is the reference's own evaluation error at q"""
    J, R, p, z, o = jacobian(m, q)
    U, sv, _ = np.linalg.svd(J, full_matrices=False)
    inv = lambda b: U @ ((U.T @ b) / (sv * sv + damp))
    y = inv(V)
    g = J.T @ y
    Jp = np.zeros((6, 7))
    om, ov, pv = np.zeros(3), np.zeros(3), J[:3] @ g
    for j in range(7):                         # (and J' by the recursion over link velocities instead of the partial derivatives)
        if j > 0:
            ov = ov + np.cross(om, o[j] - o[j - 1])
        zd = np.cross(om, z[j])
        Jp[:3, j] = np.cross(zd, p - o[j]) + np.cross(z[j], pv - ov); Jp[3:, j] = zd
        om = om + g[j] * z[j]
    return Jp.T @ y - J.T @ inv(Jp @ g + J @ (Jp.T @ y)), g


def pose_error(R, p, Rd, pd):
    return np.concatenate([p - pd, log3(R @ Rd.T)])


def tool_line_np(m, nseg, lbq, ubq, q_start, R1, p1, T_in=0.0, spec=None):
    """the plan and the record of one line as a dict: x [N][14], u [N][7], T, err_max, manip_min, s_manip, q_excess, k_fail, status, and `near`:
    the least manipulability within 10 % of manip_min, or the worst error within a factor 10 of eps"""
    sp = dict(DEFAULT_SPEC, **(spec or {}))
    damp, n_sub = sp["damp"], int(sp["n_sub"])
    N = 3 * nseg + 1
    R0, p0, w, V = line(m, q_start, R1, p1)
    if T_in > 0.0:
        T = T_in
    else:
        T = max(1.875 * np.linalg.norm(p1 - p0) / sp["tool_lin_max"], 1.875 * np.linalg.norm(w) / sp["tool_ang_max"], sp["T_min"])
    tn = time_nodes(nseg)
    x, u, manip_nodes = np.full((N, 14), np.nan), np.full((N, 7), np.nan), np.full(N, np.nan)
    v_err, u_err = np.zeros(N), np.zeros(N)      # |v - v'|, |u - u'| per node, v' and u' from field_derivative_svd: the reference's own evaluation error
    q = np.array(q_start, dtype=float)
    err_max, manip_min, s_manip, k_fail, status = 0.0, np.inf, 0.0, -1, 0

    def check(q, sg, s_here):
        nonlocal err_max, manip_min, s_manip, status
        J, R, p, _, _ = jacobian(m, q)
        en = np.linalg.norm(pose_error(R, p, R0 @ exp3(sg * w), p0 + sg * (p1 - p0)))
        G = J @ J.T
        det = np.linalg.det(G)
        mp = np.sqrt(det) if det > 0.0 and np.linalg.eigvalsh(G)[0] > 0.0 else (0.0 if det == det else np.nan)
        if not en <= err_max:
            err_max = en
        if not mp >= manip_min:
            manip_min, s_manip = mp, s_here
        if not np.isfinite(en) or not np.isfinite(mp):
            status |= NAN
        pd_ok = np.all(np.isfinite(G)) and np.linalg.eigvalsh(G + damp * np.eye(6))[0] > 0.0
        return pd_ok and en <= sp["eps"] and mp >= sp["manip_min"]

    with np.errstate(all="ignore"):
        if not check(q, 0.0, 0.0):
            k_fail = 0
        for k in range(N):
            if k_fail >= 0:
                break
            if k > 0:
                sg0, sg1 = (sigma(tn[k - 1]) if k > 1 else 0.0), (sigma(tn[k]) if k < N - 1 else 1.0)
                h = (sg1 - sg0) / n_sub
                for j in range(n_sub):
                    sg = sg1 if j == n_sub - 1 else sg0 + (sg1 - sg0) * ((j + 1) / n_sub)
                    try:
                        k1 = field(m, q, V, damp); k2 = field(m, q + 0.5 * h * k1, V, damp)
                        k3 = field(m, q + 0.5 * h * k2, V, damp); k4 = field(m, q + h * k3, V, damp)
                        q = q + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
                        Rd, pd = R0 @ exp3(sg * w), p0 + sg * (p1 - p0)
                        for _ in range(2):
                            J, R, p, _, _ = jacobian(m, q)
                            q = q - J.T @ np.linalg.solve(J @ J.T + damp * np.eye(6), pose_error(R, p, Rd, pd))
                        ok = check(q, sg, tn[k - 1] + (tn[k] - tn[k - 1]) * ((j + 1) / n_sub))
                    except np.linalg.LinAlgError:
                        ok = False
                    if not ok:
                        k_fail = k
                        break
                if k_fail >= 0:
                    break
            end = k == 0 or k == N - 1
            x[k, :7] = q
            Jk = jacobian(m, q)[0]
            manip_nodes[k] = np.sqrt(max(np.linalg.det(Jk @ Jk.T), 0.0))
            if end:
                x[k, 7:], u[k] = 0.0, 0.0
            else:
                dg, g = field_derivative(m, q, V, damp)
                sd, sdd = sigma1(tn[k]) / T, sigma2(tn[k]) / (T * T)
                x[k, 7:], u[k] = g * sd, g * sdd + dg * sd * sd
                dg2, g2 = field_derivative_svd(m, q, V, damp)
                v_err[k], u_err[k] = np.abs(g2 * sd - x[k, 7:]).max(), np.abs(g2 * sdd + dg2 * sd * sd - u[k]).max()
    if k_fail >= 0:
        status |= STOPPED
    n = k_fail if k_fail >= 0 else N
    q_excess = float(np.max(np.maximum(lbq - x[:n, :7], x[:n, :7] - ubq))) if n > 0 else -np.inf
    if q_excess > 0.0:
        status |= Q_OUT_OF_BOUNDS
    near = bool(abs(manip_min / sp["manip_min"] - 1.0) <= 0.1 or sp["eps"] / 10.0 <= err_max <= sp["eps"] * 10.0)
    return dict(x=x, u=u, T=T, err_max=err_max, manip_min=manip_min, s_manip=s_manip, q_excess=q_excess, k_fail=k_fail, status=status, near=near,
                manip_nodes=manip_nodes, v_err=v_err, u_err=u_err, V=V, R0=R0, p0=p0, w=w)


def lagrange(nseg, t):
    xi = np.array([-1.0, -0.5, 0.5, 1.0])
    s = min(max(int(np.floor(t * nseg)), 0), nseg - 1)
    xx = 2.0 * (t * nseg - s) - 1.0
    Lg = np.array([np.prod([(xx - xi[k]) / (xi[j] - xi[k]) for k in range(4) if k != j]) for j in range(4)])
    return s, Lg


def deviation_samples(m, nseg, xq, R1, p1, n_pts):
    """per sample i of n_pts + 1: (distance from the nominal position, distance from the straight line, angle from the nominal orientation);
    xq [N][7]: the position nodes"""
    R0, p0, w, V = line(m, xq[0], R1, p1)
    L = np.linalg.norm(p1 - p0)
    out = np.zeros((n_pts + 1, 3))
    for i in range(n_pts + 1):
        s = i / n_pts
        seg, Lg = lagrange(nseg, s)
        q = Lg @ xq[3 * seg:3 * seg + 4]
        R, p, _, _ = fk(m, q)
        sg = sigma(s)
        out[i, 0] = np.linalg.norm(p - (p0 + sg * (p1 - p0)))
        if L > 1e-9:                           # (a shorter line has no direction to working precision: 0 by definition)
            r = p - p0
            out[i, 1] = np.linalg.norm(r - (r @ (p1 - p0)) / (L * L) * (p1 - p0))
        D = R @ (R0 @ exp3(sg * w)).T
        v = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        out[i, 2] = np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0))
    return out


def tool_deviation_np(m, nseg, xq, R1, p1, n_pts, tol_lin=np.inf, tol_ang=np.inf):
    d = deviation_samples(m, nseg, xq, R1, p1, n_pts)
    if not np.all(np.isfinite(d)):
        return dict(lin_max=np.nan, s_lin=-1.0, perp_max=np.nan, ang_max=np.nan, s_ang=-1.0, n_over=0, status=NAN, samples=d)
    il, ia = int(np.argmax(d[:, 0])), int(np.argmax(d[:, 2]))
    n_over = int(((d[:, 0] > tol_lin) | (d[:, 2] > tol_ang)).sum())
    return dict(lin_max=d[il, 0], s_lin=il / n_pts, perp_max=d[:, 1].max(), ang_max=d[ia, 2], s_ang=ia / n_pts, n_over=n_over,
                status=TD_OVER if n_over else 0, samples=d)
