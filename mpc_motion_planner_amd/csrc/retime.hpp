// retime.hpp — what retiming of plans and of whole via-point routes (include/mpcmp_retime.h, include/mpcmp_route_retime.h) shares between the host
// entry points (mpcmp.hip), its kernels and the host statements mpcmp_retime_one / mpcmp_retime_route_one (retime.hip): the record of a grid point,
// the rows it stands for, the elimination of w over a pair of rows, the forward step and the clock, each one text for host and device.  A plan is a
// route of one leg: there is one kernel set, and the plan calls run it with M = 0.  The kernels themselves live in retime.hip, a translation unit of
// its own: nothing here is a kernel, so including this header does not change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/mpcmp.h"

namespace mpcmp {

constexpr int RT_MAX_GRID = 4096;     // n_grid
constexpr int RT_NT = 64;             // threads per workgroup of k_retime: one wave
constexpr int RT_CHUNK = 64;          // grid points per chunk, one per lane
constexpr int RT_MAX_NODES = 25;      // 3 num_seg + 1 for num_seg <= 8
constexpr int RT_MAX_ARMS = 2;
// The record of one (grid point, arm): v, a, c = RNEA(q, 0, 0), d1 = RNEA(q, v, a) - c, d2 = RNEA(q, 0, v) - c (7 each) and the arm's cap.  The 28 rows
// of the arm are formed from it and the bounds row when a pass needs them, so a chunk of 64 points costs 18 KB of LDS per arm.
constexpr int RT_V = 0, RT_A = 7, RT_C = 14, RT_D1 = 21, RT_D2 = 28, RT_CAP = 35, RT_NF = 36;
constexpr int RT_ROWS_ARM = 28;       // QDD upper 7, QDD lower 7, TAU upper 7, TAU lower 7
constexpr double RT_ZERO_A = 1e-12;

__host__ __device__ inline bool rt_finite(double x) { return x - x == 0.0; }

// the cap on x from a value v (a joint velocity, or a tool speed with lb = -inf) against [lb, ub]: +inf when v == 0 or the bound on its side is infinite
__host__ __device__ inline double rt_speed_cap(double v, double lb, double ub) {
    if (v > 0.0) { if (ub == INFINITY) return INFINITY; if (ub <= 0.0) return 0.0; const double r = ub / v; return r * r; }
    if (v < 0.0) { if (lb == -INFINITY) return INFINITY; if (lb >= 0.0) return 0.0; const double r = lb / v; return r * r; }
    return INFINITY;
}

// The record of one (point, arm) into P (field f at P[f * stride]) from the arm's v, a, the three torques c, r1 = RNEA(q, v, a), r2 = RNEA(q, 0, v) and
// the tool speeds, under the bounds row bd [58] (the layout of mpcmp_bounds).  The cap holds rate_max^2 and the QD / TOOL_LIN / TOOL_ANG groups.
__host__ __device__ inline void rt_record(const double *bd, const mpcmp_retime_spec &sp, const double *v, const double *a, const double *c,
                                          const double *r1, const double *r2, double vlin, double vang, double *P, int stride) {
    const double *lbx = bd, *ubx = bd + 14;
    double cap = sp.rate_max * sp.rate_max;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 7; j++) {
        P[(RT_V + j) * stride] = v[j]; P[(RT_A + j) * stride] = a[j]; P[(RT_C + j) * stride] = c[j];
        P[(RT_D1 + j) * stride] = r1[j] - c[j]; P[(RT_D2 + j) * stride] = r2[j] - c[j];
        if (sp.groups & (1 << MPCMP_LIM_QD)) cap = fmin(cap, rt_speed_cap(v[j], lbx[7 + j], ubx[7 + j]));
    }
    if (sp.groups & (1 << MPCMP_LIM_TOOL_LIN)) cap = fmin(cap, rt_speed_cap(vlin, -INFINITY, sp.tool_lin_max));
    if (sp.groups & (1 << MPCMP_LIM_TOOL_ANG)) cap = fmin(cap, rt_speed_cap(vang, -INFINITY, sp.tool_ang_max));
    P[RT_CAP * stride] = cap;
}

// Row rr in [0, 28) of an arm's record: A w + B x + C <= 0.  rr = 14 g + 7 side + j: g 0 QDD / 1 TAU, side 0 upper / 1 lower, joint j.  h = 1 / 2T.
// A row that is not there (group not in the mask, bound infinite) comes back as (0, 0, -1), which holds for every x and w.
__host__ __device__ inline void rt_row(const double *P, int stride, const double *bd, double h, int groups, int rr, double &A, double &B, double &C) {
    const int g = rr / 14, lower = (rr % 14) / 7, j = rr % 7;
    double a, b, c, lb, ub;
    if (g == 0) { a = P[(RT_V + j) * stride] * h; b = P[(RT_A + j) * stride]; c = 0.0; lb = bd[28 + j]; ub = bd[35 + j]; }
    else { a = P[(RT_D2 + j) * stride] * h; b = P[(RT_D1 + j) * stride]; c = P[(RT_C + j) * stride]; lb = bd[42 + j]; ub = bd[50 + j]; }
    const bool on = (groups >> (g == 0 ? MPCMP_LIM_QDD : MPCMP_LIM_TAU)) & 1;
    const double bound = lower ? lb : ub;
    if (!on || bound == INFINITY || bound == -INFINITY) { A = 0.0; B = 0.0; C = -1.0; return; }
    if (lower) { A = -a; B = -b; C = lb - c; } else { A = a; B = b; C = c - ub; }
    if (fabs(A) <= RT_ZERO_A * (fabs(B) + fabs(C) + 1.0)) A = 0.0;
}

// an interval [lo, hi] of x that rows cut down; `empty` once a row holds for no x
struct RtSet { double lo, hi; int empty; };
// a row without w: B x + C <= 0
__host__ __device__ inline void rt_cut_x(RtSet &S, double B, double C) {
    if (B > 0.0) S.hi = fmin(S.hi, -C / B);
    else if (B < 0.0) S.lo = fmax(S.lo, -C / B);
    else if (C > 0.0) S.empty = 1;
}
// w eliminated over the pair (row i with A_i > 0, row j with A_j < 0), in product form
__host__ __device__ inline void rt_cut_pair(RtSet &S, double Ai, double Bi, double Ci, double Aj, double Bj, double Cj) {
    rt_cut_x(S, Ai * Bj - Aj * Bi, Ai * Cj - Aj * Ci);
}
// the largest w a row with A > 0 allows at x
__host__ __device__ inline double rt_w_max(double A, double B, double C, double x) { return -(B * x + C) / A; }
// the time of one interval
__host__ __device__ inline double rt_dt(double T, double delta, double x0, double x1) { return 2.0 * T * delta / (sqrt(x0) + sqrt(x1)); }

// the spec a NULL pointer stands for
inline mpcmp_retime_spec rt_default_spec() {
    mpcmp_retime_spec s;
    s.tool_lin_max = s.tool_ang_max = INFINITY; s.rate_max = 1.0; s.groups = MPCMP_RT_ALL_GROUPS; s.pad = 0;
    return s;
}
inline bool rt_spec_ok(const mpcmp_retime_spec &s) {
    return s.tool_lin_max >= 0.0 && s.tool_ang_max >= 0.0 && std::isfinite(s.rate_max) && s.rate_max > 0.0 && (s.groups & ~MPCMP_RT_ALL_GROUPS) == 0;
}

// the record of a route that is not retimed (status INFEASIBLE or NAN)
__host__ __device__ inline mpcmp_route_retime rrt_failed(int status, int leg_fail, int k_fail) {
    mpcmp_route_retime r;
    r.T_new = INFINITY; r.rate_min = 0.0; r.s_slowest = -1.0; r.leg_slowest = -1; r.leg_fail = leg_fail; r.k_fail = k_fail; r.n_slowed = 0;
    r.status = status; r.pad = 0;
    return r;
}
// the record of a plan from that of its one-leg route: the same values without the leg fields
__host__ __device__ inline mpcmp_retime rt_plan_record(const mpcmp_route_retime &r) {
    mpcmp_retime p;
    p.T_new = r.T_new; p.rate_min = r.rate_min; p.s_slowest = r.s_slowest; p.k_fail = r.k_fail; p.n_slowed = r.n_slowed; p.status = r.status; p.pad = 0;
    return p;
}

// B routes of M + 1 legs each (plans: M = 0).  mdl / mstride as k_sample takes them (leg slot l, arm a: mdl + l * mstride + a); rows [B (M + 1)] or
// NULL: then `table`, the configuration's, for every leg slot; d_leg_T may be NULL.  The records go to d_route_out or, for plans (M = 0 only), to
// d_plan_out: exactly one of the two is given.
hipError_t retime_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, const mpcmp_bounds *rows,
                         const mpcmp_bounds &table, const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_retime_spec &spec,
                         double *d_prof, double *d_leg_T, mpcmp_retime *d_plan_out, mpcmp_route_retime *d_route_out, hipStream_t st);
hipError_t sample_retimed_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, int n_pts, const double *d_sx,
                                 const double *d_su, const double *d_sT, const double *d_prof, double *d_out, hipStream_t st);

}  // namespace mpcmp
