// toolpath.hpp — the rule of the tool-line moves (include/mpcmp_toolpath.h), stated once for host and device: the line and its progress law, the
// minimum-norm velocity field and its derivative along itself, the predictor / corrector continuation with its stop rule, the nodes of the plan,
// and the deviation of a plan's interpolant from the line.  k_tool_line / k_tool_deviation (toolpath.hip) and the host statements
// mpcmp_tool_line_one / mpcmp_tool_deviation_one (model_host.cpp, plain C++) run this source.  Nothing here is a kernel, and every per-lane array is
// indexed by unrolled constants only, so that on the device they live in registers.
#pragma once
#include <cmath>
#include "../../include/mpcmp.h"
#include "kinematics_host.hpp"
#include "plan_interp.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define TL_UNROLL _Pragma("unroll")
#define TL_NOUNROLL _Pragma("nounroll")
// The scheduler may not move instructions across this point.  Left alone it interleaves the seven joints' sine / cosine expansions and the square roots
// and divisions of the Cholesky rows for instruction-level parallelism, and the values in flight then exceed the registers of two waves per SIMD.
#define TL_FENCE __builtin_amdgcn_sched_barrier(0)
#else
#define TL_UNROLL
#define TL_NOUNROLL
#define TL_FENCE (void)0
#endif

namespace mpcmp_tl {

constexpr int TL_NT = 32;             // threads per workgroup of k_tool_line: one lane per line, small blocks so that a few hundred lines reach many CUs
constexpr int TD_NT = 64;             // threads per workgroup of k_tool_deviation (one wave per plan) = samples per chunk
constexpr int TL_MAX_NODES = 25;      // 3 num_seg + 1 for num_seg <= 8
constexpr int TD_MAX_PTS = 65536;
constexpr double TL_HALF_TURN = 1e-3; // |w| > pi - this is refused
constexpr double TD_POINT = 1e-9;     // a line no longer than this has no direction to working precision: the distance from it is reported as 0

MPCMP_HD bool tl_finite(double x) { return x - x == 0.0; }
MPCMP_HD double tl_nan() { return NAN; }

// the progress law and its first two derivatives
MPCMP_HD double tl_sigma(double s) { return s * s * s * (10.0 + s * (-15.0 + 6.0 * s)); }
MPCMP_HD double tl_sigma1(double s) { return s * s * (30.0 + s * (-60.0 + 30.0 * s)); }
MPCMP_HD double tl_sigma2(double s) { return s * (60.0 + s * (-180.0 + 120.0 * s)); }
// time node k of mpcmp_time_nodes
MPCMP_HD double tl_time_node(int nseg, int k) {
    int seg = k / 3, j = k % 3;
    if (seg >= nseg) { seg = nseg - 1; j = 3; }
    const double f = j == 0 ? 0.0 : (j == 1 ? 0.25 : (j == 2 ? 0.75 : 1.0));
    return (seg + f) / nseg;
}

// E = exp([w]) (Rodrigues)
MPCMP_HD void tl_exp3(const double w[3], double E[9]) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(t2);
    double a, b;                       // sin(th) / th, (1 - cos(th)) / th^2
    if (th < 1e-4) { a = 1.0 - t2 / 6.0; b = 0.5 - t2 / 24.0; }
    else { a = std::sin(th) / th; const double sh = std::sin(0.5 * th) / th; b = 2.0 * sh * sh; }
    E[0] = 1.0 - b * (w[1] * w[1] + w[2] * w[2]); E[1] = b * w[0] * w[1] - a * w[2]; E[2] = b * w[0] * w[2] + a * w[1];
    E[3] = b * w[0] * w[1] + a * w[2]; E[4] = 1.0 - b * (w[0] * w[0] + w[2] * w[2]); E[5] = b * w[1] * w[2] - a * w[0];
    E[6] = b * w[0] * w[2] - a * w[1]; E[7] = b * w[1] * w[2] + a * w[0]; E[8] = 1.0 - b * (w[0] * w[0] + w[1] * w[1]);
}

// the line from (R0, p0) to (R1, p1): w = log(R0^T R1), V = [p1 - p0; R0 w]
struct TlLine { double R0[9], p0[3], w[3], V[6], len, ang; };
// What tl_track keeps beside its registers: the line, the nominal pose of the step in hand, the RK4 sum and step length, what a step only updates at
// its end (the record's extremes, the last node's s and sigma, T), and room to park q, g and a Cholesky factor while g' is formed.  77 doubles: on the
// device one slot per lane in LDS (an odd number, so the lanes of a block read their slots from different banks), on the host a local variable.
struct TlWork { TlLine Ln; double Rd[9], pd[3], park[21], err_max, manip_min, s_manip, T, s_prev, sg_prev, h, acc[7], qs[7]; };
MPCMP_HD void tl_line(const double R0[9], const double p0[3], const double R1[9], const double p1[3], TlLine &L) {
    double D[9];
    TL_UNROLL
    for (int r = 0; r < 3; r++) {
        TL_UNROLL
        for (int c = 0; c < 3; c++) D[3 * r + c] = R0[r] * R1[c] + R0[3 + r] * R1[3 + c] + R0[6 + r] * R1[6 + c];
    }
    mpcmp_host::log3(D, L.w, &L.ang);
    TL_UNROLL
    for (int k = 0; k < 9; k++) L.R0[k] = R0[k];
    TL_UNROLL
    for (int r = 0; r < 3; r++) {
        L.p0[r] = p0[r];
        L.V[r] = p1[r] - p0[r];
        L.V[3 + r] = R0[3 * r] * L.w[0] + R0[3 * r + 1] * L.w[1] + R0[3 * r + 2] * L.w[2];
    }
    L.len = std::sqrt(L.V[0] * L.V[0] + L.V[1] * L.V[1] + L.V[2] * L.V[2]);
    L.ang = std::sqrt(L.w[0] * L.w[0] + L.w[1] * L.w[1] + L.w[2] * L.w[2]);
}
// the nominal pose at sigma
MPCMP_HD void tl_pose(const TlLine &L, double sg, double Rd[9], double pd[3]) {
    const double ws[3] = {sg * L.w[0], sg * L.w[1], sg * L.w[2]};
    double E[9];
    tl_exp3(ws, E);
    TL_UNROLL
    for (int r = 0; r < 3; r++) {
        pd[r] = L.p0[r] + sg * L.V[r];
        TL_UNROLL
        for (int c = 0; c < 3; c++) Rd[3 * r + c] = L.R0[3 * r] * E[c] + L.R0[3 * r + 1] * E[3 + c] + L.R0[3 * r + 2] * E[6 + c];
    }
}
// e = [p - pd; log(R Rd^T)]
MPCMP_HD void tl_pose_error(const double R[9], const double p[3], const double Rd[9], const double pd[3], double e[6]) {
    double D[9], th;
    TL_UNROLL
    for (int r = 0; r < 3; r++) {
        e[r] = p[r] - pd[r];
        TL_UNROLL
        for (int c = 0; c < 3; c++) D[3 * r + c] = R[3 * r] * Rd[3 * c] + R[3 * r + 1] * Rd[3 * c + 1] + R[3 * r + 2] * Rd[3 * c + 2];
    }
    mpcmp_host::log3(D, e + 3, &th);
}

// Sine and cosine of a joint angle by one argument reduction, the same arithmetic on host and device.  x = n pi/2 + r with n = rint(x 2/pi) and pi/2
// split in two (the first 33 bits, so n times it is exact for |n| < 2^20, and the rest), then the two polynomial kernels of Sun's fdlibm (k_sin.c,
// k_cos.c) on |r| <= pi/4: absolute error about 1e-16 for the |x| < 1e5 a joint angle can have.  The runtime library's sincos keeps some sixty
// vector registers busy for arguments of any size; this one needs about fifteen.
MPCMP_HD void tl_sincos(double x, double *sn, double *cs) {
    const bool sane = std::fabs(x) < 1e15;      // not NaN (a node of a stopped plan), infinite or beyond any joint angle: those give NaN, by selection
    x = sane ? x : 0.0;
    const double n = std::rint(x * 6.36619772367581382433e-01);
    const double r = (x - n * 1.57079632673412561417e+00) - n * 6.07710050650619224932e-11, z = r * r;
    const double ps = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double pc = 1.0 - 0.5 * z + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const int k = (int)(n - 4.0 * std::floor(0.25 * n));      // n mod 4 in doubles: no conversion of a large n to int
    *sn = !sane ? tl_nan() : (k == 0 ? ps : (k == 1 ? pc : (k == 2 ? -ps : -pc)));
    *cs = !sane ? tl_nan() : (k == 0 ? pc : (k == 1 ? -ps : (k == 2 ? -pc : ps)));
}
// The tool pose (R, p) and the world-aligned Jacobian J (rows [linear(3); angular(3)], row-major 6x7) at q: the chain and the columns of fk_chain and
// tool_jacobian (kinematics_host.hpp), joint by joint behind a fence, with the axes and origins kept in J's own storage: row 3 + r of column i is the
// axis, and row r holds the origin until the tool point is known: tl_chain leaves the origins in rows 0 - 2, tl_jacobian turns them into the linear
// rows.  The point of evaluation is q + c_kk kk, formed joint by joint.
MPCMP_HD void tl_chain(const mpcmp_model &M, const double *q, double c_kk, const double *kk, double J[42], double p[3], double R[9]) {
    double Rw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pw[3] = {0, 0, 0};
    const mpcmp_model *Mp = &M;
    TL_UNROLL
    for (int i = 0; i < 7; i++) {
        TL_UNROLL
        for (int r = 0; r < 3; r++) pw[r] += Rw[3 * r] * Mp->p[i][0] + Rw[3 * r + 1] * Mp->p[i][1] + Rw[3 * r + 2] * Mp->p[i][2];
        double c, s, Rj[9], Rn[9];
        tl_sincos(q[i] + c_kk * kk[i], &s, &c);
        TL_UNROLL
        for (int r = 0; r < 3; r++) {
            Rj[3 * r] = Mp->R0[i][3 * r] * c + Mp->R0[i][3 * r + 1] * s;
            Rj[3 * r + 1] = -Mp->R0[i][3 * r] * s + Mp->R0[i][3 * r + 1] * c;
            Rj[3 * r + 2] = Mp->R0[i][3 * r + 2];
        }
        TL_UNROLL
        for (int r = 0; r < 3; r++) {
            TL_UNROLL
            for (int k = 0; k < 3; k++) Rn[3 * r + k] = Rw[3 * r] * Rj[k] + Rw[3 * r + 1] * Rj[3 + k] + Rw[3 * r + 2] * Rj[6 + k];
        }
        TL_UNROLL
        for (int k = 0; k < 9; k++) Rw[k] = Rn[k];
        TL_UNROLL
        for (int r = 0; r < 3; r++) { J[(3 + r) * 7 + i] = Rw[3 * r + 2]; J[r * 7 + i] = pw[r]; }
        TL_FENCE;
    }
    TL_UNROLL
    for (int r = 0; r < 3; r++) p[r] = pw[r] + Rw[3 * r] * Mp->tool[0] + Rw[3 * r + 1] * Mp->tool[1] + Rw[3 * r + 2] * Mp->tool[2];
    TL_UNROLL
    for (int k = 0; k < 9; k++) R[k] = Rw[k];
}
MPCMP_HD void tl_jacobian(const mpcmp_model &M, const double *q, double c_kk, const double *kk, double J[42], double p[3], double R[9]) {
    tl_chain(M, q, c_kk, kk, J, p, R);
    TL_UNROLL
    for (int i = 0; i < 7; i++) {
        const double d[3] = {p[0] - J[0 * 7 + i], p[1] - J[1 * 7 + i], p[2] - J[2 * 7 + i]};
        const double z[3] = {J[3 * 7 + i], J[4 * 7 + i], J[5 * 7 + i]};
        J[0 * 7 + i] = z[1] * d[2] - z[2] * d[1];
        J[1 * 7 + i] = z[2] * d[0] - z[0] * d[2];
        J[2 * 7 + i] = z[0] * d[1] - z[1] * d[0];
    }
}

// the tool pose alone (the Jacobian's arithmetic is dead code the compiler drops)
MPCMP_HD void tl_fk(const mpcmp_model &M, const double *q, double R[9], double p[3]) {
    double J[42];
    tl_jacobian(M, q, 0.0, q, J, p, R);
}

// G = J J^T (lower triangle, packed row-wise: 21 entries)
MPCMP_HD void tl_gram(const double J[42], double G[21]) {
    TL_UNROLL
    for (int r = 0; r < 6; r++) {
        TL_UNROLL
        for (int c = 0; c <= r; c++) {
            double s = 0.0;
            TL_UNROLL
            for (int k = 0; k < 7; k++) s += J[r * 7 + k] * J[c * 7 + k];
            G[r * (r + 1) / 2 + c] = s;
        }
    }
}
// Cholesky of A + damp I IN PLACE (A packed like G comes back as L); *det = the determinant.  false: a pivot that is not > 0 (a NaN included)
MPCMP_HD bool tl_chol(double A[21], double damp, double *det) {
    bool ok = true;
    double d = 1.0;
    TL_UNROLL
    for (int r = 0; r < 6; r++) {
        TL_UNROLL
        for (int c = 0; c <= r; c++) {
            double s = A[r * (r + 1) / 2 + c] + (r == c ? damp : 0.0);
            TL_UNROLL
            for (int k = 0; k < c; k++) s -= A[r * (r + 1) / 2 + k] * A[c * (c + 1) / 2 + k];
            if (r == c) { ok = ok && (s > 0.0); d *= s; A[r * (r + 1) / 2 + r] = std::sqrt(s); }
            else A[r * (r + 1) / 2 + c] = s / A[c * (c + 1) / 2 + c];
        }
        TL_FENCE;
    }
    *det = d;
    return ok;
}
// x = (L L^T)^-1 b
MPCMP_HD void tl_chol_solve(const double L[21], const double b[6], double x[6]) {
    double y[6];
    TL_UNROLL
    for (int r = 0; r < 6; r++) {
        double s = b[r];
        TL_UNROLL
        for (int k = 0; k < r; k++) s -= L[r * (r + 1) / 2 + k] * y[k];
        y[r] = s / L[r * (r + 1) / 2 + r];
    }
    TL_FENCE;
    TL_UNROLL
    for (int r = 5; r >= 0; r--) {
        double s = y[r];
        TL_UNROLL
        for (int k = r + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + r] * x[k];
        x[r] = s / L[r * (r + 1) / 2 + r];
    }
}
// o = J^T x
MPCMP_HD void tl_jt(const double J[42], const double x[6], double o[7]) {
    TL_UNROLL
    for (int k = 0; k < 7; k++) {
        double s = 0.0;
        TL_UNROLL
        for (int r = 0; r < 6; r++) s += J[r * 7 + k] * x[r];
        o[k] = s;
    }
}

// o = J^T (J J^T + damp I)^-1 b.  false: the normal matrix is not positive definite
MPCMP_HD bool tl_dls(const double J[42], double damp, const double b[6], double o[7]) {
    double L[21], det, y[6];
    tl_gram(J, L);
    const bool ok = tl_chol(L, damp, &det);
    tl_chol_solve(L, b, y);
    tl_jt(J, y, o);
    return ok;
}

// g' = the derivative of g(q) = J^T A^-1 V along itself, A = J J^T + damp I, y = A^-1 V:  g' = a - J^T A^-1 (J' g + J a) with a = J'^T y and
// J' = sum_i (dJ / dq_i) g_i.  Column j of J': z_j' = om_j x z_j and (p - o_j)' = p' - o_j', with om_j = sum_{i<j} g_i z_i the angular velocity of the link
// that carries joint j, o_j' = o_j-1' + om_j x (o_j - o_j-1) the velocity of its origin and p' = J_lin g.  Neither J nor J' is stored: C holds the axes
// and origins of the chain (tl_chain) and a column [z_j x (p - o_j); z_j] is formed where it is used; the factor waits in `park` while the columns of
// J' are formed.  Called once per node, outside the step loop.
MPCMP_HD void tl_col(const double C[42], const double p[3], int j, double c[6], double d[3]) {
    TL_UNROLL
    for (int r = 0; r < 3; r++) { d[r] = p[r] - C[r * 7 + j]; c[3 + r] = C[(3 + r) * 7 + j]; }
    c[0] = c[4] * d[2] - c[5] * d[1]; c[1] = c[5] * d[0] - c[3] * d[2]; c[2] = c[3] * d[1] - c[4] * d[0];
}
MPCMP_HD void tl_dg(const mpcmp_model &M, const double q[7], double damp, const double V[6], double dg[7], double *park) {
    double R[9], p[3], C[42], L[21], det, y[6], g[7], c[6], d[3];
    tl_chain(M, q, 0.0, q, C, p, R);
    TL_UNROLL
    for (int k = 0; k < 21; k++) L[k] = 0.0;
    TL_UNROLL
    for (int j = 0; j < 7; j++) {
        tl_col(C, p, j, c, d);
        TL_UNROLL
        for (int r = 0; r < 6; r++) {
            TL_UNROLL
            for (int k = 0; k <= r; k++) L[r * (r + 1) / 2 + k] += c[r] * c[k];
        }
    }
    tl_chol(L, damp, &det);
    tl_chol_solve(L, V, y);
    TL_UNROLL
    for (int k = 0; k < 21; k++) park[k] = L[k];
    double pv[3] = {0.0, 0.0, 0.0};
    TL_UNROLL
    for (int j = 0; j < 7; j++) {
        tl_col(C, p, j, c, d);
        double s = 0.0;
        TL_UNROLL
        for (int r = 0; r < 6; r++) s += c[r] * y[r];
        g[j] = s;
        TL_UNROLL
        for (int r = 0; r < 3; r++) pv[r] += c[r] * s;
    }
    double a[7], bc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, om[3] = {0.0, 0.0, 0.0}, ov[3] = {0.0, 0.0, 0.0};
    TL_UNROLL
    for (int j = 0; j < 7; j++) {
        tl_col(C, p, j, c, d);
        if (j > 0) {
            const double dlt[3] = {C[0 * 7 + j] - C[0 * 7 + j - 1], C[1 * 7 + j] - C[1 * 7 + j - 1], C[2 * 7 + j] - C[2 * 7 + j - 1]};
            ov[0] += om[1] * dlt[2] - om[2] * dlt[1];
            ov[1] += om[2] * dlt[0] - om[0] * dlt[2];
            ov[2] += om[0] * dlt[1] - om[1] * dlt[0];
        }
        const double zd[3] = {om[1] * c[5] - om[2] * c[4], om[2] * c[3] - om[0] * c[5], om[0] * c[4] - om[1] * c[3]};
        const double dd[3] = {pv[0] - ov[0], pv[1] - ov[1], pv[2] - ov[2]};
        const double col[6] = {zd[1] * d[2] - zd[2] * d[1] + c[4] * dd[2] - c[5] * dd[1], zd[2] * d[0] - zd[0] * d[2] + c[5] * dd[0] - c[3] * dd[2],
                               zd[0] * d[1] - zd[1] * d[0] + c[3] * dd[1] - c[4] * dd[0], zd[0], zd[1], zd[2]};
        double s = 0.0;
        TL_UNROLL
        for (int r = 0; r < 6; r++) { s += col[r] * y[r]; bc[r] += col[r] * g[j]; }
        a[j] = s;
        TL_UNROLL
        for (int r = 0; r < 3; r++) om[r] += g[j] * c[3 + r];
        TL_FENCE;
    }
    TL_UNROLL
    for (int j = 0; j < 7; j++) {
        tl_col(C, p, j, c, d);
        TL_UNROLL
        for (int r = 0; r < 6; r++) bc[r] += c[r] * a[j];
    }
    TL_UNROLL
    for (int k = 0; k < 21; k++) L[k] = park[k];
    tl_chol_solve(L, bc, y);
    TL_UNROLL
    for (int j = 0; j < 7; j++) {
        tl_col(C, p, j, c, d);
        double s = 0.0;
        TL_UNROLL
        for (int r = 0; r < 6; r++) s += c[r] * y[r];
        dg[j] = a[j] - s;
    }
}

// the spec a NULL pointer stands for, and the rule its values must satisfy
inline mpcmp_tool_line_spec tl_default_spec() {
    mpcmp_tool_line_spec s;
    s.tool_lin_max = 1.7; s.tool_ang_max = 2.5; s.T_min = 0.2; s.damp = 1e-8; s.manip_min = 1e-3; s.eps = 1e-9; s.n_sub = 4; s.pad = 0;
    return s;
}
inline bool tl_spec_ok(const mpcmp_tool_line_spec &s) {
    auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
    return s.tool_lin_max > 0.0 && s.tool_ang_max > 0.0 && pos(s.T_min) && pos(s.damp) && pos(s.manip_min) && pos(s.eps) && s.n_sub >= 1 && s.n_sub <= 64;
}
// the duration rule
MPCMP_HD double tl_duration(const TlLine &L, const mpcmp_tool_line_spec &sp, double T_in) {
    if (T_in > 0.0) return T_in;
    return std::fmax(std::fmax(1.875 * L.len / sp.tool_lin_max, 1.875 * L.ang / sp.tool_ang_max), sp.T_min);
}

// One line, problem b of the state and control arrays X [..][N][xs] and U [..][N][us]: the arm's positions start at column col_q of a state node, its
// velocities at col_v, its accelerations at col_u of a control node (any arm layout).  The addresses are formed where a node is written, from the
// arrays' bases and b, so that no per-problem pointer lives through the continuation.  Writes every node of the arm, W.T (the duration) and *rec
// (q_excess: tl_q_excess below, once the nodes are written).  W: above.
// A step is six evaluations of one body (tool pose and Jacobian at a point, the damped solve for a right-hand side): stages 0 - 2 are stages 2 - 4 of
// classical RK4 on dq / dsigma = g(q) (autonomous: V is constant; stage 1 is the g the last step ended with), stages 3 and 4 the two corrector steps
// at the step's sigma, stage 5 the pose error, the manipulability (a J J^T that is not positive definite has 0) and g at the point reached.
MPCMP_HD void tl_track(const mpcmp_model &M, int nseg, const mpcmp_tool_line_spec &sp, const double *q_start, const double *R1, const double *p1,
                       double T_in, double *X, int xs, int col_q, int col_v, double *U, int us, int col_u, int b, mpcmp_tool_line *rec, TlWork &W) {
    const int N = 3 * nseg + 1;
    double q[7], kk[7];
    TL_UNROLL
    for (int r = 0; r < 7; r++) { q[r] = q_start[r]; kk[r] = 0.0; }
    TlLine &Ln = W.Ln;
    double *Rd = W.Rd, *pd = W.pd, *acc = W.acc;
    {
        double R0[9], p0[3];
        tl_fk(M, q, R0, p0);
        tl_line(R0, p0, R1, p1, Ln);
    }
    W.T = tl_duration(Ln, sp, T_in);
    W.err_max = 0.0; W.manip_min = INFINITY; W.s_manip = 0.0; W.s_prev = 0.0; W.sg_prev = 0.0;
    int k_fail = -1, status = tl_finite(W.T) && W.T > 0.0 ? 0 : MPCMP_TL_NAN;
    for (int k = 0; k < N; k++) {
        const int steps = k == 0 ? 1 : sp.n_sub;
        for (int j = 0; j < steps; j++) {
            {
                const double sg_k = k == N - 1 ? 1.0 : tl_sigma(tl_time_node(nseg, k));
                const double sg = j == steps - 1 ? sg_k : W.sg_prev + (sg_k - W.sg_prev) * ((double)(j + 1) / steps);
                W.h = (sg_k - W.sg_prev) / steps;
                tl_pose(Ln, sg, Rd, pd);
            }
            double en = 0.0, mp = 0.0;
            bool ok = true;
            TL_UNROLL
            for (int r = 0; r < 7; r++) acc[r] = kk[r];
            TL_NOUNROLL
            for (int st = k == 0 ? 5 : 0; st < 6; st++) {
                const double h = W.h, c = st < 2 ? 0.5 * h : (st == 2 ? h : 0.0);
                double J[42], pq[3], Rq[9], e[6], L[21], det, y[6];
                tl_jacobian(M, q, c, kk, J, pq, Rq);
                tl_pose_error(Rq, pq, Rd, pd, e);
                if (st == 5) {
                    tl_gram(J, L);
                    const bool pd0 = tl_chol(L, 0.0, &det);
                    mp = pd0 ? std::sqrt(det) : (det == det ? 0.0 : det);
                    en = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3] + e[4] * e[4] + e[5] * e[5]);
                }
                const bool corr = st == 3 || st == 4;
                TL_UNROLL
                for (int r = 0; r < 6; r++) e[r] = corr ? e[r] : Ln.V[r];
                tl_gram(J, L);
                ok = tl_chol(L, sp.damp, &det) && ok;
                tl_chol_solve(L, e, y);
                tl_jt(J, y, kk);
                const double wgt = st == 2 ? 1.0 : 2.0, step = st == 2 ? h / 6.0 : (corr ? -1.0 : 0.0);
                TL_UNROLL
                for (int r = 0; r < 7; r++) {
                    acc[r] = st < 3 ? acc[r] + wgt * kk[r] : acc[r];
                    q[r] += step * (st == 2 ? acc[r] : kk[r]);
                }
            }
            // kk holds g(q)
            if (!(en <= W.err_max)) W.err_max = en;
            if (!(mp >= W.manip_min)) { W.manip_min = mp; W.s_manip = k == 0 ? 0.0 : W.s_prev + (tl_time_node(nseg, k) - W.s_prev) * ((double)(j + 1) / steps); }
            if (!tl_finite(en) || !tl_finite(mp)) status |= MPCMP_TL_NAN;
            if (!ok || !(en <= sp.eps) || !(mp >= sp.manip_min)) { k_fail = k; break; }
        }
        if (k_fail >= 0) break;
        // node k
        const bool end = k == 0 || k == N - 1;
        const double s_k = tl_time_node(nseg, k), sg_k = k == N - 1 ? 1.0 : tl_sigma(s_k);
        const double T = W.T, sd = end ? 0.0 : tl_sigma1(s_k) / T, sdd = end ? 0.0 : tl_sigma2(s_k) / (T * T);
        // (q and g wait in the slot while g' is formed: tl_dg needs the registers)
        TL_UNROLL
        for (int r = 0; r < 7; r++) {
            X[((size_t)b * N + k) * xs + col_q + r] = q[r];
            X[((size_t)b * N + k) * xs + col_v + r] = end ? 0.0 : kk[r] * sd;
            W.qs[r] = q[r]; acc[r] = kk[r];
        }
        double dg[7];
        if (!end) tl_dg(M, W.qs, sp.damp, Ln.V, dg, W.park);
        TL_UNROLL
        for (int r = 0; r < 7; r++) {
            q[r] = W.qs[r]; kk[r] = acc[r];
            U[((size_t)b * N + k) * us + col_u + r] = end ? 0.0 : kk[r] * sdd + dg[r] * sd * sd;
        }
        W.s_prev = s_k; W.sg_prev = sg_k;
    }
    if (k_fail >= 0) {
        status |= MPCMP_TL_STOPPED;
        for (int k = k_fail; k < N; k++) {
            TL_UNROLL
            for (int r = 0; r < 7; r++) {
                X[((size_t)b * N + k) * xs + col_q + r] = tl_nan(); X[((size_t)b * N + k) * xs + col_v + r] = tl_nan();
                U[((size_t)b * N + k) * us + col_u + r] = tl_nan();
            }
        }
    }
    rec->err_max = W.err_max; rec->manip_min = W.manip_min; rec->s_manip = W.s_manip; rec->q_excess = -INFINITY; rec->k_fail = k_fail; rec->status = status;
}
// the excess of the nodes written (those before k_fail) over the position rows lbq / ubq [7], into the record tl_track left
MPCMP_HD void tl_q_excess(const double *Q, int xs, int nseg, const double *lbq, const double *ubq, mpcmp_tool_line *rec) {
    const int n = rec->k_fail >= 0 ? rec->k_fail : 3 * nseg + 1;
    double ex = -INFINITY;
    for (int k = 0; k < n; k++) {
        TL_UNROLL
        for (int r = 0; r < 7; r++) { const double v = Q[(size_t)xs * k + r]; ex = std::fmax(ex, std::fmax(lbq[r] - v, v - ubq[r])); }
    }
    rec->q_excess = ex;
    if (ex > 0.0) rec->status |= MPCMP_TL_Q_OUT_OF_BOUNDS;
}

// ---- the deviation of a plan from its line ----
// the line of a plan: from the tool pose of node 0 (Q: the arm's positions there) to (R1, p1)
MPCMP_HD void tl_line_of_plan(const mpcmp_model &M, const double *Q, const double *R1, const double *p1, TlLine &Ln) {
    double q[7], R0[9], p0[3];
    TL_UNROLL
    for (int r = 0; r < 7; r++) q[r] = Q[r];
    tl_fk(M, q, R0, p0);
    tl_line(R0, p0, R1, p1, Ln);
}
// sample i of n_pts: the distance from the nominal position, the distance from the straight line, the angle from the nominal orientation
MPCMP_HD void tl_dev_sample(const mpcmp_model &M, const TlLine &Ln, int nseg, const double *Q, int xs, int i, int n_pts, double *dlin, double *dperp,
                            double *dang) {
    const double s = (double)i / n_pts;
    double Lg[4], q[7];
    const int seg = mpcmp_plan::lagrange_segment(nseg, s, Lg);
    mpcmp_plan::interp_q(Q, xs, seg, Lg, q);
    double R[9], p[3], Rd[9], pd[3];
    tl_fk(M, q, R, p);
    tl_pose(Ln, tl_sigma(s), Rd, pd);
    const double d[3] = {p[0] - pd[0], p[1] - pd[1], p[2] - pd[2]};
    *dlin = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (Ln.len > TD_POINT) {
        const double r0[3] = {p[0] - Ln.p0[0], p[1] - Ln.p0[1], p[2] - Ln.p0[2]};
        const double al = (r0[0] * Ln.V[0] + r0[1] * Ln.V[1] + r0[2] * Ln.V[2]) / (Ln.len * Ln.len);
        const double c[3] = {r0[0] - al * Ln.V[0], r0[1] - al * Ln.V[1], r0[2] - al * Ln.V[2]};
        *dperp = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    } else *dperp = (*dlin == *dlin) ? 0.0 : *dlin;
    // the angle of D = R Rd^T from its skew part and its trace (atan2: exact to rounding at small angles, where acos of the trace alone is not)
    double D[9];
    TL_UNROLL
    for (int r = 0; r < 3; r++) {
        TL_UNROLL
        for (int c = 0; c < 3; c++) D[3 * r + c] = R[3 * r] * Rd[3 * c] + R[3 * r + 1] * Rd[3 * c + 1] + R[3 * r + 2] * Rd[3 * c + 2];
    }
    const double vx = D[7] - D[5], vy = D[2] - D[6], vz = D[3] - D[1];
    *dang = std::atan2(0.5 * std::sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (D[0] + D[4] + D[8] - 1.0));
}
// what a thread (or the host loop) keeps over its samples, and how two of them combine: the larger value, of equal ones the lower sample index
struct TlDevAcc { double lin, perp, ang; int i_lin, i_ang, n_over, nan; };
MPCMP_HD void tl_dev_init(TlDevAcc &A) { A.lin = A.perp = A.ang = -1.0; A.i_lin = A.i_ang = 0x7FFFFFFF; A.n_over = 0; A.nan = 0; }
MPCMP_HD void tl_dev_fold(TlDevAcc &A, int i, double dlin, double dperp, double dang, double tol_lin, double tol_ang) {
    if (!tl_finite(dlin) || !tl_finite(dperp) || !tl_finite(dang)) { A.nan = 1; return; }
    if (dlin > A.lin || (dlin == A.lin && i < A.i_lin)) { A.lin = dlin; A.i_lin = i; }
    if (dang > A.ang || (dang == A.ang && i < A.i_ang)) { A.ang = dang; A.i_ang = i; }
    A.perp = std::fmax(A.perp, dperp);
    if (dlin > tol_lin || dang > tol_ang) A.n_over++;
}
MPCMP_HD void tl_dev_merge(TlDevAcc &A, double lin, int i_lin, double perp, double ang, int i_ang, int n_over, int nan) {
    if (lin > A.lin || (lin == A.lin && i_lin < A.i_lin)) { A.lin = lin; A.i_lin = i_lin; }
    if (ang > A.ang || (ang == A.ang && i_ang < A.i_ang)) { A.ang = ang; A.i_ang = i_ang; }
    A.perp = std::fmax(A.perp, perp);
    A.n_over += n_over; A.nan |= nan;
}
MPCMP_HD mpcmp_tool_dev tl_dev_record(const TlDevAcc &A, int n_pts) {
    mpcmp_tool_dev r;
    if (A.nan) { r.lin_max = r.perp_max = r.ang_max = tl_nan(); r.s_lin = r.s_ang = -1.0; r.n_over = 0; r.status = MPCMP_TL_NAN; return r; }
    r.lin_max = A.lin; r.s_lin = (double)A.i_lin / n_pts; r.perp_max = A.perp; r.ang_max = A.ang; r.s_ang = (double)A.i_ang / n_pts;
    r.n_over = A.n_over; r.status = A.n_over > 0 ? MPCMP_TD_OVER : 0;
    return r;
}

// the value checks of one problem that the host entry points share (mpcmp_tool_line_batch, mpcmp_tool_line_one): nullptr, or what is wrong
inline const char *tl_check_problem(const mpcmp_model &M, const double *q_start, const double *R1, const double *p1, double T_in) {
    for (int k = 0; k < 7; k++) if (!std::isfinite(q_start[k])) return "an input value is not finite";
    for (int k = 0; k < 9; k++) if (!std::isfinite(R1[k])) return "an input value is not finite";
    for (int k = 0; k < 3; k++) if (!std::isfinite(p1[k])) return "an input value is not finite";
    if (!std::isfinite(T_in)) return "an input value is not finite";
    const double *r = R1;
    double dev = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dev = std::fmax(dev, std::fabs(r[i] * r[j] + r[3 + i] * r[3 + j] + r[6 + i] * r[6 + j] - (i == j ? 1.0 : 0.0)));
    const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
    if (dev > 1e-6 || !(det > 0.0)) return "R1 is not a rotation";
    double R0[9], p0[3];
    tl_fk(M, q_start, R0, p0);
    TlLine Ln;
    tl_line(R0, p0, R1, p1, Ln);
    if (Ln.ang > M_PI - TL_HALF_TURN) return "the rotation from the start pose to R1 is within 1e-3 of a half turn: the geodesic is ambiguous";
    return nullptr;
}

#ifdef __HIPCC__
// mdl: the arm's model (one for every problem: the rule is kinematic); rows [B] or NULL: then `table`, the configuration's, for everyone.  col_q /
// col_v: the arm's first position / velocity column in a state node of nx doubles, col_u in a control node of nu
struct TlQRows { double lb[7], ub[7]; };      // the position rows of the configuration
hipError_t tool_line_launch(const mpcmp_model *mdl, int nseg, int B, const mpcmp_bounds *rows, const mpcmp_bounds &table, int nx, int nu, int col_q,
                            int col_v, int col_u, const double *d_q, const double *d_R1, const double *d_p1, const double *d_Tin,
                            const mpcmp_tool_line_spec &spec, double *d_sx, double *d_su, double *d_sT, mpcmp_tool_line *d_out, hipStream_t st);
hipError_t tool_deviation_launch(const mpcmp_model *mdl, int nseg, int B, int nx, int col_q, const double *d_sx, const double *d_R1, const double *d_p1,
                                 int n_pts, double tol_lin, double tol_ang, mpcmp_tool_dev *d_out, hipStream_t st);
#endif

}  // namespace mpcmp_tl
