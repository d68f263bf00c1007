// sample_device.hpp — one row of get_MPC_trajectory (motionPlanner.hpp:99-116) as a device function: the state and control of a trajectory at a
// normalised time, the node interpolant of plan_interp.hpp, and the RNEA torque.  k_sample (leaf_kernels.hpp) and k_sample_route (route.hip) both
// call it, so that a route sample is the row a plain sample of its leg gives; the other device readers of a plan interpolate with the two pieces it
// is made of.  Nothing here is a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "plan_interp.hpp"
#include "rbd_device.hpp"

namespace mpcmp {

using mpcmp_plan::lagrange_segment;

// interp_qva (plan_interp.hpp) on the device, plus sc [14] = sine, cosine of q.  Joint by joint, each sine / cosine beside the sums it follows: the
// order the kernels' register budgets were measured with (with the sines after all the sums k_traj_stats and k_sample_retimed spill 8 B more)
__device__ __forceinline__ void interp_joints(const double *Q, const double *V, int xs, const double *A, int us, int s, const double *Lg,
                                              double *q, double *v, double *a, double *sc) {
#pragma unroll
    for (int r = 0; r < 7; r++) {
        q[r] = mpcmp_plan::interp_channel(Q + r, xs, s, Lg);
        v[r] = mpcmp_plan::interp_channel(V + r, xs, s, Lg);
        a[r] = mpcmp_plan::interp_channel(A + r, us, s, Lg);
        sincos(q[r], &sc[2 * r], &sc[2 * r + 1]);
    }
}

// X [N][14], U [N][7] of one single-arm trajectory with N = 3 nseg + 1 nodes; t in [0, 1]; o [29]: o[1..28] = q, qd, qdd, tau (o[0], the time
// column, is the caller's)
__device__ __forceinline__ void sample_row(const mpcmp_model *mdl, int nseg, const double *X, const double *U, double t, double *o) {
    double Lg[4];
    const int s = lagrange_segment(nseg, t, Lg);
    double q[7], v[7], a[7], tau[7], sc[14];
    interp_joints(X, X + 7, 14, U, 7, s, Lg, q, v, a, sc);
    rnea_dir<false>(mdl, sc, v, a, 0, 0, tau, nullptr);
#pragma unroll
    for (int r = 0; r < 7; r++) { o[1 + r] = q[r]; o[8 + r] = v[r]; o[15 + r] = a[r]; o[22 + r] = tau[r]; }
}

}  // namespace mpcmp
