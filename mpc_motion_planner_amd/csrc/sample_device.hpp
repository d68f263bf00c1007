// sample_device.hpp — one row of get_MPC_trajectory (motionPlanner.hpp:99-116) as a device function: the state and control of a trajectory at a
// normalised time, Lagrange interpolation on the segment, and the RNEA torque.  k_sample (solver_kernels.hpp) and k_sample_route (route.hip) both
// call it, so that a route sample is the row a plain sample of its leg gives.  Nothing here is a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "rbd_device.hpp"

namespace mpcmp {

// X [N][14], U [N][7] of one single-arm trajectory with N = 3 nseg + 1 nodes; t in [0, 1]; o [29]: o[1..28] = q, qd, qdd, tau (o[0], the time
// column, is the caller's)
__device__ __forceinline__ void sample_row(const mpcmp_model *mdl, int nseg, const double *X, const double *U, double t, double *o) {
    const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
    int s = (int)floor(t * nseg);
    if (s >= nseg) s = nseg - 1;
    if (s < 0) s = 0;
    const double xx = 2.0 * (t * nseg - s) - 1.0;
    double Lg[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double v = 1.0;
#pragma unroll
        for (int k = 0; k < 4; k++) if (k != j) v *= (xx - xi[k]) / (xi[j] - xi[k]);
        Lg[j] = v;
    }
    double q[7], v[7], a[7], tau[7], sc[14];
#pragma unroll
    for (int r = 0; r < 7; r++) {
        q[r] = v[r] = a[r] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            q[r] += Lg[j] * X[14 * (3 * s + j) + r];
            v[r] += Lg[j] * X[14 * (3 * s + j) + 7 + r];
            a[r] += Lg[j] * U[7 * (3 * s + j) + r];
        }
        sincos(q[r], &sc[2 * r], &sc[2 * r + 1]);
    }
    rnea_dir<false>(mdl, sc, v, a, 0, 0, tau, nullptr);
#pragma unroll
    for (int r = 0; r < 7; r++) { o[1 + r] = q[r]; o[8 + r] = v[r]; o[15 + r] = a[r]; o[22 + r] = tau[r]; }
}

}  // namespace mpcmp
