// sample_device.hpp — one row of get_MPC_trajectory (motionPlanner.hpp:99-116) as a device function: the state and control of a trajectory at a
// normalised time, Lagrange interpolation on the segment, and the RNEA torque.  k_sample (solver_kernels.hpp) and k_sample_route (route.hip) both
// call it, so that a route sample is the row a plain sample of its leg gives; k_limits (limits.hip) interpolates with the two pieces it is made
// of.  Nothing here is a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "rbd_device.hpp"

namespace mpcmp {

// The segment of the normalised time t in [0, 1] and the four Lagrange weights of its nodes 3 s .. 3 s + 3: the interpolation rule of every sampler
// (k_sample, k_sample_route, k_limits)
__device__ __forceinline__ int lagrange_segment(int nseg, double t, double *Lg) {
    const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
    int s = (int)floor(t * nseg);
    if (s >= nseg) s = nseg - 1;
    if (s < 0) s = 0;
    const double xx = 2.0 * (t * nseg - s) - 1.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double v = 1.0;
#pragma unroll
        for (int k = 0; k < 4; k++) if (k != j) v *= (xx - xi[k]) / (xi[j] - xi[k]);
        Lg[j] = v;
    }
    return s;
}

// q, qd, qdd [7] of one arm on segment s with the weights Lg, and sc [14] = sine, cosine of q.  Q / V / A point at the arm's seven positions /
// velocities / accelerations in node 0; xs / us doubles lie between two nodes of the state / control arrays (any arm layout)
__device__ __forceinline__ void interp_joints(const double *Q, const double *V, int xs, const double *A, int us, int s, const double *Lg,
                                              double *q, double *v, double *a, double *sc) {
#pragma unroll
    for (int r = 0; r < 7; r++) {
        q[r] = v[r] = a[r] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            q[r] += Lg[j] * Q[xs * (3 * s + j) + r];
            v[r] += Lg[j] * V[xs * (3 * s + j) + r];
            a[r] += Lg[j] * A[us * (3 * s + j) + r];
        }
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
