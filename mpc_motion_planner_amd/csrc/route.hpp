// route.hpp — via-point routes (include/mpcmp.h, "via-point routes"): what the host entry points (mpcmp.hip), the kernels (route.hip) and the host
// helpers mpcmp_route_via_velocity / mpcmp_route_locate share.  The arithmetic is in __host__ __device__ functions: the helpers and the kernels are
// one text.  All of it is FP64, and every sum runs sequentially in leg order: a route's records do not depend on the batch around it.
// The kernels themselves live in route.hip, a translation unit of their own: nothing here is a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "../../include/mpcmp.h"

namespace mpcmp {

__host__ __device__ inline double route_nan() {
    const unsigned long long u = 0x7FF8000000000000ull;
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// Chord rule: the pass-through velocity V [7 narm] at the via Pi between its neighbours Pa and Pb, within the limits of `row` (the per-arm tables
// apply to each arm's seven columns).  The last line keeps |V_j| <= vlim_j against the rounding of s * d_j.
__host__ __device__ inline void route_via_velocity(const double *Pa, const double *Pi, const double *Pb, const mpcmp_bounds *row, int narm, double speed,
                                                   double *V) {
    const int nq = 7 * narm;
    double s = INFINITY;
    for (int j = 0; j < nq; j++) {
        const int c = j % 7;
        const double vlim = fmin(row->ubx[7 + c], -row->lbx[7 + c]), alim = fmin(row->ubu[c], -row->lbu[c]);
        const double a = Pi[j] - Pa[j], b = Pb[j] - Pi[j];
        const double d = (a * b > 0.0 && vlim > 0.0 && alim > 0.0) ? 0.5 * (a + b) : 0.0;
        V[j] = d;
        if (d != 0.0) {
            const double cap = fmin(vlim, sqrt(2.0 * alim * fmin(fabs(a), fabs(b))));
            const double r = cap / fabs(d);
            if (r < s) s = r;
        }
    }
    for (int j = 0; j < nq; j++) {
        const double d = V[j];
        if (d == 0.0 || !(s < INFINITY)) { V[j] = 0.0; continue; }      // (no joint moves through; or every moving joint is unlimited: nothing to scale to)
        const double vlim = fmin(row->ubx[7 + j % 7], -row->lbx[7 + j % 7]);
        const double v = speed * s * d;
        V[j] = fabs(v) > vlim ? copysign(vlim, v) : v;
    }
}

// Leg and normalised time of the route time t: E_m = the sequential prefix sums of T [n]; the smallest m with t < E_m, n - 1 if there is none;
// tau = clamp((t - E_{m-1}) / T_m, 0, 1), 0 where the quotient is no number (a last leg of length 0)
__host__ __device__ inline void route_locate(int n, const double *T, double t, int *leg, double *tau) {
    double Ep = 0.0;
    int m = 0;
    for (;;) {
        const double E = Ep + T[m];
        if (t < E || m == n - 1) break;
        Ep = E; m++;
    }
    const double x = (t - Ep) / T[m];
    *leg = m;
    *tau = !(x > 0.0) ? 0.0 : (x > 1.0 ? 1.0 : x);
}

// maxima and minima that keep a NaN once they have met one
__host__ __device__ inline void route_max(double &m, double v) { if (v > m || v != v) m = v; }
__host__ __device__ inline void route_min(double &m, double v) { if (v < m || v != v) m = v; }

// the legs of ONE route (nl = M + 1 of them, the pointers at its first leg) joined into one record of each kind; clr / rclr may be NULL
__host__ __device__ inline void route_join_one(int nl, int N, int nx, int nu, const double *sx, const double *su, const double *sT, const mpcmp_info *info,
                                               const mpcmp_clearance *clr, double *rT, mpcmp_info *rinfo, mpcmp_route_seam *seam, mpcmp_clearance *rclr) {
    const int bad = MPCMP_STATUS_NAN | MPCMP_STATUS_NOT_PD | MPCMP_STATUS_XCH_DEAD | MPCMP_STATUS_OUTSIDE_TOL | MPCMP_STATUS_T_OUT_OF_BOX;
    mpcmp_info r = info[0];
    mpcmp_route_seam s;
    s.state_jump_inf = 0.0; s.acc_jump_inf = 0.0; s.leg_longest = 0;
    s.leg_first_bad = (info[0].status & bad) ? 0 : -1;
    double T = sT[0], Tl = sT[0];
    for (int m = 1; m < nl; m++) {
        const mpcmp_info &i = info[m];
        T += sT[m];
        route_max(r.viol_l1, i.viol_l1); route_max(r.defect_inf, i.defect_inf); route_max(r.path_viol_inf, i.path_viol_inf);
        route_max(r.term_err_inf, i.term_err_inf); route_min(r.last_alpha, i.last_alpha);
        if (i.sqp_iters > r.sqp_iters) r.sqp_iters = i.sqp_iters;
        r.qp_iters_total += i.qp_iters_total; r.qp_capped += i.qp_capped; r.status |= i.status;
        if (sT[m] > Tl) { Tl = sT[m]; s.leg_longest = m; }
        if (s.leg_first_bad < 0 && (i.status & bad)) s.leg_first_bad = m;
        const double *xa = sx + ((size_t)m * N - 1) * nx, *xb = sx + (size_t)m * N * nx;        // last node of leg m - 1, node 0 of leg m
        for (int c = 0; c < nx; c++) route_max(s.state_jump_inf, fabs(xa[c] - xb[c]));
        const double *ua = su + ((size_t)m * N - 1) * nu, *ub = su + (size_t)m * N * nu;
        for (int c = 0; c < nu; c++) route_max(s.acc_jump_inf, fabs(ua[c] - ub[c]));
    }
    r.T = T;
    *rT = T; *rinfo = r; *seam = s;
    if (!clr || !rclr) return;
    mpcmp_clearance o;
    o.d_min = INFINITY; o.t_min = -1.0; o.t_first = -1.0; o.sphere = -1; o.other = 0; o.n_hit = 0; o.status = 0;
    double E = 0.0;                                    // the sum of the earlier legs' T
    for (int m = 0; m < nl; m++) {
        const mpcmp_clearance &c = clr[m];
        o.status |= c.status; o.n_hit += c.n_hit;
        if (c.sphere >= 0 && c.d_min < o.d_min) { o.d_min = c.d_min; o.t_min = c.t_min + E; o.sphere = c.sphere; o.other = c.other; }
        if (o.t_first < 0.0 && c.t_first >= 0.0) o.t_first = c.t_first + E;
        E += sT[m];
    }
    if (o.status & MPCMP_CLR_NAN) { o.d_min = route_nan(); o.t_min = -1.0; o.t_first = -1.0; o.sphere = -1; o.other = 0; o.n_hit = 0; }
    *rclr = o;
}

// launchers (route.hip); every pointer is a device pointer
// rows: the bound rows in force [L] or NULL (then cfg_row, the configuration's tables, for every leg slot)
hipError_t route_legs_launch(int B, int M, int narm, const double *x0, const double *via, const double *via_qd, const double *speed, const double *xf,
                             const mpcmp_bounds *rows, const mpcmp_bounds &cfg_row, double *leg_x0, double *leg_xf, double *via_qd_out, hipStream_t st);
hipError_t route_join_launch(int B, int M, int N, int narm, const double *sx, const double *su, const double *sT, const mpcmp_info *info,
                             const mpcmp_clearance *clr, double *rT, mpcmp_info *rinfo, mpcmp_route_seam *seam, mpcmp_clearance *rclr, hipStream_t st);
// mdl / mstride as k_sample takes them: the payload row of a LEG SLOT
hipError_t route_sample_launch(const mpcmp_model *mdl, int mstride, int nseg, int B, int M, int n_pts, const double *sx, const double *su, const double *sT,
                               double *out, hipStream_t st);

}  // namespace mpcmp
