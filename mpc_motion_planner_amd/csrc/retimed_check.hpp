// retimed_check.hpp — what the limit checker of retimed plans and routes (include/mpcmp_retimed_check.h) shares between the host entry points
// (mpcmp.hip), its kernels and the host statement mpcmp_limits_retimed_one (retimed_check.hip): the place of a sample on a profile (profile_place.hpp,
// plain C++, read by the host-only unit as well) and the record a finished accumulator stands for, each one text for host and device.  The excess,
// ratio and tie rules are those of limits.hpp and the sizes of a profile those of retime.hpp; both are included and not changed.  Nothing here is a kernel, so including this header does not change what any other
// translation unit compiles to.
#pragma once
#include "limits.hpp"
#include "retime.hpp"
#include "profile_place.hpp"

namespace mpcmp {

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
