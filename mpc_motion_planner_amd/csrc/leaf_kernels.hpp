// leaf_kernels.hpp — the non-template kernels behind the single-purpose entry points of the C-ABI unit (mpcmp.hip): inverse dynamics, sampling and
// point evaluation of a solution, the receding-horizon loop's state advance and update, and the per-trajectory checks.  A non-template __global__ is
// defined by every translation unit that includes its header: mpcmp.hip is the only one that includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "rbd_device.hpp"
#include "sample_device.hpp"
#include "solver_types.hpp"

namespace mpcmp {

// ------------------------------------------------------------------------------------------------
// leaf kernels
// (mstride: models per point behind mdl — 0, or narm with per-problem payload rows, WS::mstride; point / problem i reads arm 0 of row i.  Every
//  leaf kernel below that evaluates dynamics takes one)
__global__ __launch_bounds__(64) void k_rnea_batch(const mpcmp_model *mdl, int mstride, int n, const double *q, const double *v, const double *a,
                             double *tau) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mdl += (size_t)i * mstride;
    double sc[14], vv[7], aa[7], t[7];
#pragma unroll
    for (int j = 0; j < 7; j++) { sincos(q[7 * i + j], &sc[2 * j], &sc[2 * j + 1]); vv[j] = v[7 * i + j]; aa[j] = a[7 * i + j]; }
    rnea_dir<false>(mdl, sc, vv, aa, 0, 0, t, nullptr);
#pragma unroll
    for (int j = 0; j < 7; j++) tau[7 * i + j] = t[j];
}

// get_MPC_trajectory<n_pts> (motionPlanner.hpp:99-116): Lagrange interpolation on the segment + RNEA
__global__ __launch_bounds__(128) void k_sample(const mpcmp_model *mdl, int mstride, int nseg, int B, int n_pts, const double *sx, const double *su,
                         const double *sT, double *out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * (n_pts + 1);
    if (gid >= total) return;
    const int b = (int)(gid / (n_pts + 1)), ip = (int)(gid % (n_pts + 1));
    mdl += (size_t)b * mstride;
    const int N = 3 * nseg + 1;
    const double t = (double)ip / n_pts;
    double *o = out + (size_t)gid * 29;
    sample_row(mdl, nseg, sx + (size_t)b * 14 * N, su + (size_t)b * 7 * N, t, o);
    o[0] = t * sT[b];
}


// MotionPlanner::get_MPC_point (motionPlanner.hpp:118-128) for one physical time per problem, including the reference's clamp
// (time >= T: the normalised time becomes T, not 1), plus the RNEA torque.  out [B][28] = q(7), v(7), a(7), tau(7).
__global__ __launch_bounds__(64) void k_mpc_point(const mpcmp_model *mdl, int mstride, int nseg, int B, const double *sx, const double *su, const double *sT,
                                                  const double *time, double *out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    mdl += (size_t)b * mstride;
    const int N = 3 * nseg + 1;
    const double T = sT[b];
    const double t = (time[b] < T) ? time[b] / T : T;
    double Lg[4];
    const int s = lagrange_segment(nseg, t, Lg);
    const double *X = sx + (size_t)b * 14 * N, *U = su + (size_t)b * 7 * N;
    double q[7], v[7], a[7], tau[7], sc[14];
    interp_joints(X, X + 7, 14, U, 7, s, Lg, q, v, a, sc);
    rnea_dir<false>(mdl, sc, v, a, 0, 0, tau, nullptr);
    double *o = out + (size_t)b * 28;
#pragma unroll
    for (int r = 0; r < 7; r++) { o[r] = q[r]; o[7 + r] = v[r]; o[14 + r] = a[r]; o[21 + r] = tau[r]; }
}

// Receding horizon, one thread per instance: x0 <- MPC solution evaluated at physical time dt (MotionPlanner::get_MPC_point,
// motionPlanner.hpp:118-128), and ARRIVAL: the reference's loop has no end (the caller decides), and an OCP whose start lies in its
// terminal box degenerates (T -> lbT = 0).  Rule, the same in the oracle (orc_rh_advance):
//   * retired already                          -> nothing;
//   * the solve failed hard or left the box of T -> the state is held (there is no trajectory to follow; the next k_init starts afresh);
//   * T <= dt: the plan ends within this control period -> the instance follows it to its end (last node) and is retired;
//   * else the state advances by dt (for dt < T the clamp of get_MPC_point never acts); if the new state lies inside the terminal box
//     |x - x_target| <= eps_target, the instance is retired as well.
// A retired instance keeps its state, its last solution and its record (status |= MPCMP_STATUS_ARRIVED) and is not re-solved (MPCMP_RETIRED).
// count[0] += instances solved in this step (not retired at its start), count[1] += instances retired by this step.
__global__ __launch_bounds__(256) void k_advance(int nseg, int nx, int B, double dt, double eps_target, const double *sx, const double *sT,
                                                 const int *status, const double *xf, double *x0, int *retired, mpcmp_info *info,
                                                 unsigned long long *count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (retired[b]) return;
    atomicAdd(&count[0], 1ull);
    if (status[b] & MPCMP_ST_FAILED) return;
    const int N = 3 * nseg + 1;
    const double T = sT[b];
    const double *X = sx + (size_t)b * N * nx;
    double *xo = x0 + (size_t)b * nx;
    bool arrive = false;
    if (T <= dt) {
        for (int r = 0; r < nx; r++) xo[r] = X[(size_t)(N - 1) * nx + r];
        arrive = true;
    } else {
        double w[4];
        const double *Xs = X + (size_t)(3 * lagrange_segment(nseg, dt / T, w)) * nx;       // the first node of the segment
        double far = 0.0;
        for (int r = 0; r < nx; r++) {
            const double acc = mpcmp_plan::interp_channel(Xs + r, nx, 0, w);
            xo[r] = acc;
            far = fmax(far, fabs(acc - xf[(size_t)b * nx + r]));
        }
        arrive = far <= eps_target;
    }
    if (arrive) {
        retired[b] = 1;
        if (info) info[b].status |= MPCMP_STATUS_ARRIVED;
        atomicAdd(&count[1], 1ull);
    }
}

// Receding horizon, between two steps (mpcmp_rh_update[_device]), one thread per listed instance b = idx[i] (idx null: b = i): the measured state
// x [n][nx] and / or the target xf [n][nx] (either may be null) overwrite the loop's current state x0 / target xt of b
// (MotionPlanner::set_current_state / set_target_state, motionPlanner.cpp:27-53).  What the next solve of b starts from:
//   * live, a state only                -> nothing more: k_init re-guesses from the previous solution with the new head (solve_trajectory(false));
//   * live, a target or `restart`       -> MPCMP_ST_RESTART: the driver's start guess and zero multipliers (k_init / k_init_m: prev_bad);
//   * retired (arrived)                 -> revived: retired := 0, MPCMP_STATUS_ARRIVED leaves its record now, count[1] -= 1, and a restart.
// The revival is an atomic exchange, so that an index listed twice (the device entry point cannot check) is counted once.
__global__ __launch_bounds__(256) void k_rh_update(int nx, int n, const int *idx, const double *x, const double *xf, int restart,
                                                   double *x0, double *xt, int *retired, int *status, mpcmp_info *info,
                                                   unsigned long long *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = idx ? idx[i] : i;
    if (x) for (int r = 0; r < nx; r++) x0[(size_t)b * nx + r] = x[(size_t)i * nx + r];
    if (xf) for (int r = 0; r < nx; r++) xt[(size_t)b * nx + r] = xf[(size_t)i * nx + r];
    bool rs = restart || xf;
    if (atomicExch(&retired[b], 0) != 0) {
        atomicAnd(&info[b].status, ~MPCMP_STATUS_ARRIVED);
        atomicAdd(&count[1], ~0ull);                          // (- 1 modulo 2^64)
        rs = true;
    }
    if (rs) atomicOr(&status[b], MPCMP_ST_RESTART);
}


// Per-trajectory checks of examples/benchmark.cpp:58-160 in one pass: resample at n_pts+1 uniform times (interpolation + RNEA),
// min / max of the 28 channels, terminal error, and the four pass flags (jerk, linear / angular task velocity, table
// collision).  One workgroup per trajectory; out [B][74] = mins(28) | maxs(28) | x(T) - x_target (14) | flags (4, 1 = pass).
__global__ __launch_bounds__(256) void k_traj_stats(const mpcmp_model *mdl, int mstride, int nseg, int n_pts, const double *sx, const double *su,
                                                    const double *sT, const double *xf, double max_lin, double max_ang,
                                                    const double *jerk10 /*[7] = 10 x max_jerk*/, double *out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *smp = lds;                          // [n_pts+1][28]
    __shared__ int fl[4];
    const int b = blockIdx.x, tid = threadIdx.x, N = 3 * nseg + 1;
    mdl += (size_t)b * mstride;
    const double *X = sx + (size_t)b * 14 * N, *U = su + (size_t)b * 7 * N;
    const double T = sT[b];
    if (tid < 4) fl[tid] = 1;
    __syncthreads();
    for (int ip = tid; ip <= n_pts; ip += blockDim.x) {
        double Lg[4];
        const int s = lagrange_segment(nseg, (double)ip / n_pts, Lg);
        double q[7], v[7], a[7], tau[7], sc[14];
        interp_joints(X, X + 7, 14, U, 7, s, Lg, q, v, a, sc);
        rnea_dir<false>(mdl, sc, v, a, 0, 0, tau, nullptr);
        V3 pt, vl, va;
        fk_task_velocity(mdl, sc, v, &pt, &vl, &va);
        if (sqrt(vl.x * vl.x + vl.y * vl.y + vl.z * vl.z) > max_lin) fl[1] = 0;     // benchmark.cpp:139-142
        if (sqrt(va.x * va.x + va.y * va.y + va.z * va.z) > max_ang) fl[2] = 0;     // :143-146
        if (pt.z < 0.0) fl[3] = 0;                                                  // :149-155
        double *o = smp + (size_t)ip * 28;
#pragma unroll
        for (int r = 0; r < 7; r++) { o[r] = q[r]; o[7 + r] = v[r]; o[14 + r] = a[r]; o[21 + r] = tau[r]; }
    }
    __syncthreads();
    const double dT = T / n_pts;                                                     // time(nPoints)/nPoints, :121
    for (int ip = 1 + tid; ip <= n_pts; ip += blockDim.x)
        for (int r = 0; r < 7; r++)
            if (fabs((smp[(size_t)ip * 28 + 14 + r] - smp[(size_t)(ip - 1) * 28 + 14 + r]) / dT) > jerk10[r]) fl[0] = 0;   // :126-133
    double *o = out + (size_t)b * 74;
    if (tid < 28) {
        double mn = smp[tid], mx = smp[tid];
        for (int ip = 1; ip <= n_pts; ip++) { const double v = smp[(size_t)ip * 28 + tid]; mn = fmin(mn, v); mx = fmax(mx, v); }
        o[tid] = mn; o[28 + tid] = mx;
    }
    if (tid < 14) o[56 + tid] = smp[(size_t)n_pts * 28 + tid] - xf[(size_t)b * 14 + tid];   // :176-179
    __syncthreads();
    if (tid < 4) o[70 + tid] = (double)fl[tid];
}

}  // namespace mpcmp
