// retimed_check.hpp — what the limit checker of retimed plans and routes (include/mpcmp_retimed_check.h) shares between the host entry points
// (mpcmp.hip), its kernels and the host statement mpcmp_limits_retimed_one (retimed_check.hip): the place of a sample on a profile and the record a
// finished accumulator stands for, each one text for host and device.  The excess, ratio and tie rules are those of limits.hpp and the sizes of a
// profile those of retime.hpp; both are included and not changed.  Nothing here is a kernel, so including this header does not change what any other
// translation unit compiles to.
#pragma once
#include "limits.hpp"
#include "retime.hpp"

namespace mpcmp {

// Where the time t of a leg lies on that leg's profile pf [n + 1][2] = (t_k, x_k), by the retimed-sample rule of mpcmp_retime.h: the interval
// k = the largest k <= n - 1 with t_k <= t (a bisection, at most 12 steps), then lambda, s and w_k.  `last`: the sample is the end of the plan or
// route (s = 1 with lambda = sqrt(x_n) and the w of the last interval).  h = 1 / 2T.
struct RcPlace { double lam, s, wh; };          // wh = w_k / 2T
__host__ __device__ inline RcPlace rc_place(const double *pf, int n, double t, double h, bool last) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pf[2 * mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int k = last ? n - 1 : lo;
    const double tk = pf[2 * k], xk = pf[2 * k + 1], x1 = pf[2 * k + 3], lk = sqrt(xk), w = (x1 - xk) * n;
    RcPlace p;
    p.lam = lk + w * (t - tk) * h;
    p.s = (double)k / n + (t - tk) * (lk + p.lam) * h;
    if (last) { p.lam = sqrt(x1); p.s = 1.0; }
    p.s = fmin(fmax(p.s, 0.0), 1.0);
    p.wh = w * h;
    return p;
}

// the record of a finished accumulator: times are (double)sample / n_pts * Tn, the retimed clock
__host__ __device__ inline mpcmp_limits rc_record(const LimAcc &A, const mpcmp_limits_spec &sp, int n_pts, double Tn) {
    mpcmp_limits r;
    r.status = 0; r.pad = 0;
    for (int g = 0; g < MPCMP_LIM_GROUPS; g++) {
        if (A.nan) { r.excess[g] = NAN; r.t_at[g] = -1.0; r.channel[g] = -1; continue; }
        r.excess[g] = A.ex[g];
        if (A.key[g] == LIM_NO_KEY) { r.t_at[g] = -1.0; r.channel[g] = -1; }
        else { r.t_at[g] = ((double)(A.key[g] >> 4) / n_pts) * Tn; r.channel[g] = (int)(A.key[g] & 0xFu); }
        if (A.ex[g] > sp.tol[g]) r.status |= 1 << g;
    }
    if (A.nan) { r.stretch = 1.0; r.t_first = -1.0; r.n_viol = 0; r.status = MPCMP_LIM_NAN; }
    else {
        r.stretch = lim_stretch(A.r);
        r.t_first = A.first != LIM_NO_SAMPLE ? ((double)A.first / n_pts) * Tn : -1.0;
        r.n_viol = A.n_viol;
    }
    return r;
}

// B routes of M + 1 legs each (plans: M = 0).  mdl / mstride as k_sample takes them (leg slot l, arm a: mdl + l * mstride + a); rows [B (M + 1)] or
// NULL: then `table`, the configuration's, for everyone; d_Tnew may be NULL
hipError_t limits_retimed_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, int n_pts,
                                 const mpcmp_bounds *rows, const mpcmp_bounds &table, const double *d_sx, const double *d_su, const double *d_sT,
                                 const double *d_prof, const mpcmp_limits_spec &spec, mpcmp_limits *d_out, double *d_Tnew, hipStream_t st);
hipError_t profile_scale_launch(int L, int n_grid, const double *d_factor, double *d_prof, hipStream_t st);

}  // namespace mpcmp
