// profile_place.hpp — where a time lies on a retime profile (include/mpcmp_retime.h, "Retimed sample"), stated once for every reader of a profile:
// the limit checker of retimed plans (retimed_check.hpp) and the checks in a moving world (moving_rule.hpp).  Plain C++, so that the host-only unit
// (model_host.cpp) reads the same source as the kernels.  Nothing here is a kernel.
#pragma once
#include <cmath>

// (the macro of kinematics_host.hpp, token for token, so that either file may come first)
#ifndef MPCMP_HD
#ifdef __HIPCC__
#define MPCMP_HD __host__ __device__ inline
#else
#define MPCMP_HD inline
#endif
#endif

namespace mpcmp {

// Where the time t of a leg lies on that leg's profile pf [n + 1][2] = (t_k, x_k), by the retimed-sample rule of mpcmp_retime.h: the interval
// k = the largest k <= n - 1 with t_k <= t (a bisection, at most 12 steps), then lambda, s and w_k.  `last`: the sample is the end of the plan or
// route (s = 1 with lambda = sqrt(x_n) and the w of the last interval).  h = 1 / 2T.
struct RcPlace { double lam, s, wh; };          // wh = w_k / 2T
MPCMP_HD RcPlace rc_place(const double *pf, int n, double t, double h, bool last) {
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

}  // namespace mpcmp
