"""Inverse dynamics from the energies of the chain: a reference that is NOT a Newton-Euler recursion (plain numpy).

The oracle (oracle/rbd.c) and the kernels (csrc/rbd_device.hpp) both propagate velocities, accelerations and forces along the chain.  This module
never does: it writes down the kinetic energy  1/2 qd^T M(q) qd  and the potential energy  U(q)  of the seven bodies from forward kinematics, and
takes the torques from Lagrange's equations,

    tau = M qdd + (dM/dt) qd - 1/2 grad_q (qd^T M qd) + grad_q U,        dM/dt = sum_k dM/dq_k qd_k,

with every derivative by the complex step  f'(x) = Im f(x + i h) / h,  h = 1e-30: no subtraction, so no cancellation, and the truncation error
(h^2) is far below one unit in the last place.  For that the forward kinematics are written for complex q: no abs, no conjugating transpose, no
arctan2 anywhere on that path.

    M(q)  = sum_i  m_i Jv_i^T Jv_i + Jw_i^T (R_i I_i R_i^T) Jw_i         Jv_i, Jw_i: Jacobians of body i's centre of mass and rotation
    U(q)  = - sum_i m_i g . c_i(q)                                       g: the model's full gravity vector

A model is the struct of include/mpcmp.h: joint frame i = R0_i Rz(q_i) at p_i in frame i - 1 (frame -1 = world); body i rides on frame i with
centre of mass com_i and inertia I_i about it, both in frame i; tool and link8 are points of frame 7.

Everything is batched over the leading dimensions of q [..., 7].

Measured accuracy (tests/test_rbd_reference_host.py::test_reference_states_its_own_accuracy, the Panda, three general robots and the tilted-gravity
robot, 20 samples each with velocities and accelerations up to the Panda limits, x86-64 80-bit long double):

    complex128 against clongdouble, largest absolute difference:   tau 2.4e-14 N m (|tau| up to 78),  M 1.6e-15,  dtau/dqd 1.3e-14
    dtau/dq (Richardson, long double, steps 2^-17 and 2^-18): largest error estimate 3.1e-10 (on the Panda), median 2.7e-11, entries up to 53.
    The estimate is the distance between the second-order level at the smaller step and the fourth-order level, so it bounds the error of the
    LOWER level; the fourth-order value is limited by the rounding of tau in long double instead (about 1e-17 / h = 1e-12): against the oracle's
    directional derivatives it differs by 1e-12 on these samples
"""
import numpy as np

H = 1e-30                     # complex step
FD_H = 2.0 ** -17             # larger step of the Richardson pair of dtau_dq (the smaller one is half of it)
FIELDS = ("R0", "p", "mass", "com", "I", "tool", "link8", "gravity")


def model_fields(m):
    """the fields of a ctypes Model (capi.Model, oracle_py.Model) as numpy arrays"""
    return dict(R0=np.array(m.R0).reshape(7, 3, 3), p=np.array(m.p).reshape(7, 3), mass=np.array(m.mass[:]), com=np.array(m.com).reshape(7, 3),
                I=np.array(m.I).reshape(7, 3, 3), tool=np.array(m.tool[:]), link8=np.array(m.link8[:]), gravity=np.array(m.gravity[:]))


def _cross(a, b):
    """a x b along the last axis (complex-safe: products and differences only)"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


class Reference:
    """real: np.float64 or np.longdouble, the precision everything is evaluated in (complex128 / clongdouble on the complex-step path)"""

    def __init__(self, R0, p, mass, com, I, tool, link8, gravity, real=np.float64):
        self.real = real
        self.cplx = np.result_type(real, np.complex64).type
        for k, v in zip(FIELDS, (R0, p, mass, com, I, tool, link8, gravity)):
            setattr(self, k, np.asarray(v, dtype=real))
        self.h = real(H)

    @classmethod
    def from_model(cls, m, real=np.float64):
        return cls(real=real, **model_fields(m))

    # ---- kinematics ----
    def frames(self, q):
        """world rotation [..., 7, 3, 3] and origin [..., 7, 3] of every joint frame: R_i = R_{i-1} R0_i Rz(q_i), p_i = p_{i-1} + R_{i-1} p_i"""
        q = np.asarray(q)
        dt = np.result_type(q.dtype, self.real)
        lead = q.shape[:-1]
        Rp = np.broadcast_to(np.eye(3, dtype=dt), lead + (3, 3)); pp = np.zeros(lead + (3,), dtype=dt)
        Rw, pw = [], []
        for i in range(7):
            c, s = np.cos(q[..., i]), np.sin(q[..., i])
            Rz = np.zeros(lead + (3, 3), dtype=dt)
            Rz[..., 0, 0] = c; Rz[..., 0, 1] = -s; Rz[..., 1, 0] = s; Rz[..., 1, 1] = c; Rz[..., 2, 2] = 1.0
            pi = pp + np.einsum("...ij,j->...i", Rp, self.p[i])
            Ri = np.einsum("...ij,jk,...kl->...il", Rp, self.R0[i], Rz)
            Rw.append(Ri); pw.append(pi)
            Rp, pp = Ri, pi
        return np.stack(Rw, axis=-3), np.stack(pw, axis=-2)

    def _point_jacobian(self, Rw, pw, point, last):
        """Jacobian [..., 3, 7] of a world point carried by frame `last`: column j = z_j x (point - p_j) for j <= last, else 0"""
        z = Rw[..., :, :, 2]                                               # [..., 7, 3] joint axes in the world
        J = _cross(z, point[..., None, :] - pw)                            # [..., 7, 3]
        keep = (np.arange(7) <= last).astype(self.real)
        return np.swapaxes(J * keep[:, None], -1, -2)

    def fk(self, q):
        """dict: R [..., 7, 3, 3], p [..., 7, 3] of the joint frames; tool, link8 [..., 3]; J [..., 6, 7] the world-aligned tool Jacobian
        [linear; angular] from the axes and lever arms"""
        Rw, pw = self.frames(q)
        tool = pw[..., 6, :] + np.einsum("...ij,j->...i", Rw[..., 6, :, :], self.tool)
        link8 = pw[..., 6, :] + np.einsum("...ij,j->...i", Rw[..., 6, :, :], self.link8)
        J = np.concatenate([self._point_jacobian(Rw, pw, tool, 6), np.swapaxes(Rw[..., :, :, 2], -1, -2)], axis=-2)
        return dict(R=Rw, p=pw, tool=tool, link8=link8, J=J)

    def frame_jacobian(self, q, off):
        """world-aligned [linear; angular] Jacobian [..., 6, 7] of the point `off` of frame 7"""
        Rw, pw = self.frames(q)
        pt = pw[..., 6, :] + np.einsum("...ij,j->...i", Rw[..., 6, :, :], np.asarray(off, dtype=self.real))
        return np.concatenate([self._point_jacobian(Rw, pw, pt, 6), np.swapaxes(Rw[..., :, :, 2], -1, -2)], axis=-2)

    def body_coms(self, q):
        Rw, pw = self.frames(q)
        return Rw, pw, pw + np.einsum("...bij,bj->...bi", Rw, self.com)

    # ---- energies ----
    def mass_matrix(self, q):
        """M [..., 7, 7] = sum_i m_i Jv_i^T Jv_i + Jw_i^T (R_i I_i R_i^T) Jw_i  (plain transposes: analytic in q)"""
        Rw, pw, c = self.body_coms(q)
        z = Rw[..., :, :, 2]
        M = 0.0
        for i in range(7):
            Jv = self._point_jacobian(Rw, pw, c[..., i, :], i)                                     # [..., 3, 7]
            Jw = np.swapaxes(z * (np.arange(7) <= i).astype(self.real)[:, None], -1, -2)            # [..., 3, 7]
            Iw = np.einsum("...ij,jk,...lk->...il", Rw[..., i, :, :], self.I[i], Rw[..., i, :, :])  # R I R^T
            M = M + self.mass[i] * np.einsum("...ki,...kj->...ij", Jv, Jv) + np.einsum("...ki,...kl,...lj->...ij", Jw, Iw, Jw)
        return M

    def potential(self, q):
        """U [...] = - sum_i m_i g . c_i(q)"""
        _, _, c = self.body_coms(q)
        return -np.einsum("b,...bd,d->...", self.mass, c, self.gravity)

    # ---- Lagrange ----
    def _velocity_term(self, q, qd):
        """c(q, qd) = (dM/dt) qd - 1/2 grad_q (qd^T M qd), quadratic in qd; q, qd real [..., 7]"""
        ih = self.h * self.cplx(1j)
        Q = np.concatenate([(q + ih * qd)[..., None, :], q[..., None, :] + ih * np.eye(7, dtype=self.real)], axis=-2)      # [..., 8, 7]
        dM = self.mass_matrix(Q).imag / self.h
        Mdot_qd = np.einsum("...ij,...j->...i", dM[..., 0, :, :], qd)
        grad = np.einsum("...i,...kij,...j->...k", qd, dM[..., 1:, :, :], qd)
        return Mdot_qd - 0.5 * grad

    def gravity_term(self, q):
        ih = self.h * self.cplx(1j)
        return self.potential(q[..., None, :] + ih * np.eye(7, dtype=self.real)).imag / self.h

    def tau(self, q, qd, qdd):
        q, qd, qdd = (np.asarray(v, dtype=self.real) for v in (q, qd, qdd))
        M = self.mass_matrix(q)
        return np.einsum("...ij,...j->...i", M, qdd) + self._velocity_term(q, qd) + self.gravity_term(q)

    def dtau_dqdd(self, q):
        return self.mass_matrix(np.asarray(q, dtype=self.real))

    def dtau_dqd(self, q, qd):
        """exact: the velocity term is a quadratic form in qd, so d c / d qd_j = c(q, qd + e_j) - c(q, qd) - c(q, e_j).  [..., 7, 7]"""
        q, qd = np.asarray(q, dtype=self.real), np.asarray(qd, dtype=self.real)
        E = np.eye(7, dtype=self.real)
        V = np.concatenate([qd[..., None, :], qd[..., None, :] + E, np.broadcast_to(E, qd.shape[:-1] + (7, 7))], axis=-2)       # [..., 15, 7]
        c = self._velocity_term(np.broadcast_to(q[..., None, :], V.shape), V)
        return np.swapaxes(c[..., 1:8, :] - c[..., 0:1, :] - c[..., 8:15, :], -1, -2)

    def dtau_dq(self, q, qd, qdd, h=FD_H):
        """(d tau / d q [..., 7, 7], error estimate [..., 7, 7]): central differences of tau at the steps h and h / 2, evaluated in long double,
        Richardson-extrapolated to fourth order; the estimate is |fourth-order level - second-order level at h / 2|"""
        ld = self if self.real is np.longdouble else Reference(*(getattr(self, k) for k in FIELDS), real=np.longdouble)
        q, qd, qdd = (np.asarray(v, dtype=np.longdouble) for v in (q, qd, qdd))
        E = np.eye(7, dtype=np.longdouble)
        steps = np.concatenate([h * E, -h * E, 0.5 * h * E, -0.5 * h * E])                          # [28, 7]
        t = ld.tau(q[..., None, :] + steps, qd[..., None, :], qdd[..., None, :])                    # [..., 28, 7]
        D1 = (t[..., 0:7, :] - t[..., 7:14, :]) / (2 * np.longdouble(h))
        D2 = (t[..., 14:21, :] - t[..., 21:28, :]) / np.longdouble(h)
        R = (4 * D2 - D1) / 3
        est = np.maximum(R - D2, D2 - R)
        return np.swapaxes(R, -1, -2).astype(self.real), np.swapaxes(est, -1, -2).astype(np.float64)

    def constraints(self, x, u, quirk=1):
        """g [..., 8], G [..., 8, 22], the Richardson estimate of the dq block [..., 7, 7]: the layout of orc_eval_constraints.  Torque rows
        [dq | dqd | M symmetric | dT]; with the quirk dT_i = sum_j dv_ij qd_j + sum_{j >= i} M_ij qdd_j (oracle/rbd.c, the loop that fills row[21]),
        without it 0; row 7 = tool height and the z row of the tool Jacobian"""
        x, u = np.asarray(x, dtype=self.real), np.asarray(u, dtype=self.real)
        q, qd = x[..., :7], x[..., 7:]
        f = self.fk(q)
        M = self.mass_matrix(q)
        dv = self.dtau_dqd(q, qd)
        dq, est = self.dtau_dq(q, qd, u)
        g = np.concatenate([self.tau(q, qd, u), f["tool"][..., 2:3]], axis=-1)
        G = np.zeros(x.shape[:-1] + (8, 22), dtype=self.real)
        G[..., :7, 0:7] = dq; G[..., :7, 7:14] = dv; G[..., :7, 14:21] = 0.5 * (M + np.swapaxes(M, -1, -2))
        if quirk:
            G[..., :7, 21] = np.einsum("...ij,...j->...i", dv, qd) + np.einsum("...ij,...j->...i", np.triu(M), u)
        G[..., 7, 0:7] = f["J"][..., 2, :]
        return g, G, est


# ---- the bars every comparison with this reference uses (those of tests/test_gpu_parity.py between the kernels and the oracle) ----
TAU_TOL = 1e-11


def jac_tol(G_ref):
    return 1e-10 * (1.0 + np.abs(G_ref).max())


def assert_constraints_close(g, G, g_ref, G_ref, est, what=""):
    """g [8], G [8, 22] against the reference's: 1e-11 on the values, 1e-10 (1 + max |G|) on the Jacobian; on the dq block that bar or, entry by
    entry, ten times the Richardson estimate where that is larger"""
    assert np.abs(g - g_ref).max() < TAU_TOL, (what, np.abs(g - g_ref).max())
    bar = jac_tol(G_ref)
    d = np.abs(G - G_ref)
    assert d[:, 7:].max() < bar, (what, d[:, 7:].max(), bar)
    assert d[7, :7].max() < bar, (what, d[7, :7].max(), bar)
    assert np.all(d[:7, :7] < np.maximum(bar, 10.0 * est)), (what, d[:7, :7].max(), bar, est.max())
