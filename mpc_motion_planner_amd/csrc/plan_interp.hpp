// plan_interp.hpp — what a finished plan is between its nodes, stated once for host and device: on each of its nseg segments the cubic Lagrange
// interpolant through the segment's four nodes, which lie at xi = -1, -1/2, 1/2, 1 of the segment (get_MPC_trajectory, motionPlanner.hpp:99-116).
// Every reader of a plan runs this source: the samplers, the point evaluation, the receding-horizon advance, the trajectory statistics, clearance,
// limits, retiming and its checker, the tool deviation, and the host statements that mirror them; so two readers cannot disagree about a plan in the
// last bit.  Plain C++ (model_host.cpp reads it without the HIP runtime's header); nothing here is a kernel.
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
// the sums below run over constant indices on the device, so that a caller's per-lane arrays stay in registers
#if defined(__HIP_DEVICE_COMPILE__)
#define PLAN_UNROLL _Pragma("unroll")
#else
#define PLAN_UNROLL
#endif

namespace mpcmp_plan {

// collocation node j = 0 .. 3 of a segment, in the segment's coordinate
MPCMP_HD double node_xi(int j) {
    const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
    return xi[j];
}

// the normalised time of node k = 0 .. 3 nseg of a discretisation (what mpcmp_time_nodes tabulates); a node two segments share is the later one's first
MPCMP_HD double node_time(int nseg, int k) {
    int s = k / 3, j = k % 3;
    if (s >= nseg) { s = nseg - 1; j = 3; }
    return (s + 0.5 * (node_xi(j) + 1.0)) / nseg;
}

// The segment s of the normalised time t and the four weights Lg of its nodes 3 s .. 3 s + 3.  t outside [0, 1] extrapolates the first / last
// segment; t must be a number (the conversion to int is not defined otherwise)
MPCMP_HD int lagrange_segment(int nseg, double t, double *Lg) {
    int s = (int)std::floor(t * nseg);
    if (s >= nseg) s = nseg - 1;
    if (s < 0) s = 0;
    const double xx = 2.0 * (t * nseg - s) - 1.0;
    PLAN_UNROLL
    for (int j = 0; j < 4; j++) {
        double v = 1.0;
        PLAN_UNROLL
        for (int k = 0; k < 4; k++) if (k != j) v *= (xx - node_xi(k)) / (node_xi(j) - node_xi(k));
        Lg[j] = v;
    }
    return s;
}

// The four weights of the normalised time t on a segment s THE CALLER NAMES: the cubic of segment s, also at a t that is the segment's end (where
// lagrange_segment would answer with the next segment) or outside it
MPCMP_HD void lagrange_on_segment(int nseg, int s, double t, double *Lg) {
    const double xx = 2.0 * (t * nseg - s) - 1.0;
    PLAN_UNROLL
    for (int j = 0; j < 4; j++) {
        double v = 1.0;
        PLAN_UNROLL
        for (int k = 0; k < 4; k++) if (k != j) v *= (xx - node_xi(k)) / (node_xi(j) - node_xi(k));
        Lg[j] = v;
    }
}

// ... and the weights dLg of the DERIVATIVE of that cubic in normalised time (d xi / d t = 2 nseg): sum_j dLg[j] C[node 3 s + j] is the slope of the
// position interpolant itself, which is not the velocity channel of a plan
MPCMP_HD void lagrange_derivative_on_segment(int nseg, int s, double t, double *dLg) {
    const double xx = 2.0 * (t * nseg - s) - 1.0;
    PLAN_UNROLL
    for (int j = 0; j < 4; j++) {
        double d = 0.0;
        PLAN_UNROLL
        for (int m = 0; m < 4; m++) {
            if (m == j) continue;
            double v = 1.0 / (node_xi(j) - node_xi(m));
            PLAN_UNROLL
            for (int k = 0; k < 4; k++) if (k != j && k != m) v *= (xx - node_xi(k)) / (node_xi(j) - node_xi(k));
            d += v;
        }
        dLg[j] = 2.0 * nseg * d;
    }
}

// One scalar channel on segment s with the weights Lg: C points at the channel in node 0, `stride` doubles lie between two nodes
MPCMP_HD double interp_channel(const double *C, int stride, int s, const double *Lg) {
    double c = 0.0;
    PLAN_UNROLL
    for (int j = 0; j < 4; j++) c += Lg[j] * C[stride * (3 * s + j)];
    return c;
}

// q [7] of one arm: Q points at the arm's seven positions in node 0, xs doubles lie between two nodes of the state array (any arm layout)
MPCMP_HD void interp_q(const double *Q, int xs, int s, const double *Lg, double *q) {
    PLAN_UNROLL
    for (int r = 0; r < 7; r++) q[r] = interp_channel(Q + r, xs, s, Lg);
}

// q, qd, qdd [7] of one arm: Q / V / A point at the arm's seven positions / velocities / accelerations in node 0; xs / us doubles lie between two
// nodes of the state / control arrays
MPCMP_HD void interp_qva(const double *Q, const double *V, int xs, const double *A, int us, int s, const double *Lg, double *q, double *v, double *a) {
    PLAN_UNROLL
    for (int r = 0; r < 7; r++) {
        q[r] = interp_channel(Q + r, xs, s, Lg);
        v[r] = interp_channel(V + r, xs, s, Lg);
        a[r] = interp_channel(A + r, us, s, Lg);
    }
}

}  // namespace mpcmp_plan
