// route_retime.hpp — what route retiming (include/mpcmp_route_retime.h) shares between the host entry points (mpcmp.hip), its kernels and the host
// statement mpcmp_retime_route_one (route_retime.hip).  The arithmetic of a grid point is that of retime.hpp, which this header includes and does
// not change; nothing here is a kernel, so including it does not change what any other translation unit compiles to.
#pragma once
#include "retime.hpp"

namespace mpcmp {

// the record of a route that is not retimed (status INFEASIBLE or NAN)
__host__ __device__ inline mpcmp_route_retime rrt_failed(int status, int leg_fail, int k_fail) {
    mpcmp_route_retime r;
    r.T_new = INFINITY; r.rate_min = 0.0; r.s_slowest = -1.0; r.leg_slowest = -1; r.leg_fail = leg_fail; r.k_fail = k_fail; r.n_slowed = 0;
    r.status = status; r.pad = 0;
    return r;
}

// mdl / mstride as k_sample takes them (leg slot l, arm a: mdl + l * mstride + a); rows [L] or NULL: then `table`, the configuration's, for every leg
// slot; d_leg_T may be NULL
hipError_t retime_route_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, const mpcmp_bounds *rows,
                               const mpcmp_bounds &table, const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_retime_spec &spec,
                               double *d_prof, double *d_leg_T, mpcmp_route_retime *d_out, hipStream_t st);
hipError_t sample_retimed_route_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, int n_pts, const double *d_sx,
                                       const double *d_su, const double *d_sT, const double *d_prof, double *d_out, hipStream_t st);

}  // namespace mpcmp
