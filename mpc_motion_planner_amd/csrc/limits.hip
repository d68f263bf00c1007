// limits.hip — the between-node limit checker (include/mpcmp.h, "limits between the nodes"): per trajectory the excess of every group over its
// bounds at the uniform samples of the interpolant, the stretch that cures the kinematic groups, and the host helper that needs no context.
// A translation unit of its own, so that the register-bound QP kernels of solver.hip compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "limits.hpp"
#include "sample_device.hpp"
#include "kinematics_host.hpp"
#include "rnea_host.hpp"

namespace mpcmp {

// One workgroup per trajectory.  Staged in LDS once: the nodes of the trajectory (x and u, at most 25 x 42 doubles) and the bounds row of the
// problem.  Then one thread per sample, strided over the n_pts + 1 samples, and for every arm in turn the work of k_traj_stats: the Lagrange rule of
// sample_row (lagrange_segment, interp_joints), sine / cosine, the RNEA torque with the arm's model, one forward-kinematics pass for the tool
// position and twist; lim_fold_arm compares.  Nothing of a sample is stored: a thread keeps its LimAcc in registers over all its samples, and one
// workgroup reduction at the end orders the (excess, key) pairs by lim_better, takes the maxima of the ratios (exact, so order-free), sums the
// counts and takes the minimum of the first indices.  No atomics: the record does not depend on the launch or on the batch.
__global__ __launch_bounds__(LIM_NT) void k_limits(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int n_pts,
                                                   const mpcmp_bounds *__restrict__ rows, mpcmp_bounds table, const double *__restrict__ sx,
                                                   const double *__restrict__ su, const double *__restrict__ sT, mpcmp_limits_spec sp,
                                                   mpcmp_limits *__restrict__ out) {
    __shared__ double nodes[LIM_MAX_NODES * 21 * LIM_MAX_ARMS];      // x [N][14 narm], then u [N][7 narm]
    __shared__ double bd[58];
    constexpr int NW = LIM_NT / 64;
    __shared__ double red_e[NW][MPCMP_LIM_GROUPS], red_r[NW][4];
    __shared__ unsigned red_k[NW][MPCMP_LIM_GROUPS];
    __shared__ int red_i[NW][3];
    const int b = blockIdx.x, tid = threadIdx.x, N = 3 * nseg + 1, nq = 7 * narm;
    double *Xs = nodes, *Us = nodes + 2 * nq * N;
    const double *X = sx + (size_t)b * N * 2 * nq, *U = su + (size_t)b * N * nq;
    for (int e = tid; e < 2 * nq * N; e += LIM_NT) Xs[e] = X[e];
    for (int e = tid; e < nq * N; e += LIM_NT) Us[e] = U[e];
    {
        const double *row = reinterpret_cast<const double *>(rows + b), *tab = reinterpret_cast<const double *>(&table);
        for (int e = tid; e < 58; e += LIM_NT) bd[e] = rows ? row[e] : tab[e];
    }
    __syncthreads();

    LimAcc A;
    lim_init(A);
    for (int ip = tid; ip <= n_pts; ip += LIM_NT) {
        double Lg[4];
        const int s = lagrange_segment(nseg, (double)ip / n_pts, Lg);
        bool over = false;
        for (int a = 0; a < narm; a++) {
            const mpcmp_model *M = mdl + (size_t)b * mstride + a;
            double q[7], v[7], ac[7], tau[7], sc[14];
            interp_joints(Xs + 7 * a, Xs + nq + 7 * a, 2 * nq, Us + 7 * a, nq, s, Lg, q, v, ac, sc);
            rnea_dir<false>(M, sc, v, ac, 0, 0, tau, nullptr);
            V3 pt, vl, va;
            fk_task_velocity(M, sc, v, &pt, &vl, &va);
            over |= lim_fold_arm(A, bd, sp, ip, a, q, v, ac, tau, pt.z, sqrt(vl.x * vl.x + vl.y * vl.y + vl.z * vl.z),
                                 sqrt(va.x * va.x + va.y * va.y + va.z * va.z));
        }
        lim_count(A, ip, over);
    }

    // workgroup reduction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int g = 0; g < MPCMP_LIM_GROUPS; g++) {
            const double oe = __shfl_down(A.ex[g], off);
            const unsigned ok = __shfl_down(A.key[g], off);
            if (lim_better(oe, ok, A.ex[g], A.key[g])) { A.ex[g] = oe; A.key[g] = ok; }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) A.r[k] = fmax(A.r[k], __shfl_down(A.r[k], off));
        A.n_viol += __shfl_down(A.n_viol, off);
        const int of = __shfl_down(A.first, off);
        A.first = of < A.first ? of : A.first;
        A.nan |= __shfl_down(A.nan, off);
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
#pragma unroll
        for (int g = 0; g < MPCMP_LIM_GROUPS; g++) { red_e[w][g] = A.ex[g]; red_k[w][g] = A.key[g]; }
#pragma unroll
        for (int k = 0; k < 4; k++) red_r[w][k] = A.r[k];
        red_i[w][0] = A.n_viol; red_i[w][1] = A.first; red_i[w][2] = A.nan;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; w++) {
#pragma unroll
            for (int g = 0; g < MPCMP_LIM_GROUPS; g++)
                if (lim_better(red_e[w][g], red_k[w][g], A.ex[g], A.key[g])) { A.ex[g] = red_e[w][g]; A.key[g] = red_k[w][g]; }
#pragma unroll
            for (int k = 0; k < 4; k++) A.r[k] = fmax(A.r[k], red_r[w][k]);
            A.n_viol += red_i[w][0];
            A.first = red_i[w][1] < A.first ? red_i[w][1] : A.first;
            A.nan |= red_i[w][2];
        }
        const double T = sT[b];
        mpcmp_limits r;
        r.status = 0; r.pad = 0;
#pragma unroll
        for (int g = 0; g < MPCMP_LIM_GROUPS; g++) {
            if (A.nan) { r.excess[g] = __longlong_as_double(0x7FF8000000000000ll); r.t_at[g] = -1.0; r.channel[g] = -1; continue; }
            r.excess[g] = A.ex[g];
            if (A.key[g] == LIM_NO_KEY) { r.t_at[g] = -1.0; r.channel[g] = -1; }
            else { r.t_at[g] = ((double)(A.key[g] >> 4) / n_pts) * T; r.channel[g] = (int)(A.key[g] & 0xFu); }
            if (A.ex[g] > sp.tol[g]) r.status |= 1 << g;
        }
        if (A.nan) { r.stretch = 1.0; r.t_first = -1.0; r.n_viol = 0; r.status = MPCMP_LIM_NAN; }
        else {
            r.stretch = lim_stretch(A.r);
            r.t_first = A.first != LIM_NO_SAMPLE ? ((double)A.first / n_pts) * T : -1.0;
            r.n_viol = A.n_viol;
        }
        out[b] = r;
    }
}

hipError_t limits_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int n_pts, const mpcmp_bounds *rows, const mpcmp_bounds &table,
                         const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_limits_spec &spec, mpcmp_limits *d_out, hipStream_t st) {
    if (narm < 1 || narm > LIM_MAX_ARMS || nseg < 1 || 3 * nseg + 1 > LIM_MAX_NODES || n_pts < 1 || n_pts > LIM_MAX_PTS || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_limits, dim3(B), dim3(LIM_NT), 0, st, mdl, mstride, narm, nseg, n_pts, rows, table, d_sx, d_su, d_sT, spec, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host helper (no GPU) ----

extern "C" int mpcmp_limits_config(const mpcmp_model *models, int narm, const mpcmp_bounds *row, const mpcmp_limits_spec *spec, const double *q,
                                   const double *qd, const double *qdd, double *excess, int *channel, double *ratios) {
    if (!models || narm < 1 || narm > LIM_MAX_ARMS || !row || !q || !qd || !qdd || !excess) return MPCMP_EINVAL;
    const mpcmp_limits_spec sp = spec ? *spec : lim_default_spec();
    if (!lim_spec_ok(sp)) return MPCMP_EINVAL;
    LimAcc A;
    lim_init(A);
    for (int a = 0; a < narm; a++) {
        double tau[7], J[42], p[3], R[9], tw[6];
        mpcmp_host::rnea_host(models[a], q + 7 * a, qd + 7 * a, qdd + 7 * a, tau);
        mpcmp_host::tool_jacobian(models[a], q + 7 * a, J, p, R);
        for (int r = 0; r < 6; r++) { tw[r] = 0.0; for (int j = 0; j < 7; j++) tw[r] += J[7 * r + j] * qd[7 * a + j]; }
        lim_fold_arm(A, reinterpret_cast<const double *>(row), sp, 0, a, q + 7 * a, qd + 7 * a, qdd + 7 * a, tau, p[2],
                     std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]), std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]));
    }
    for (int g = 0; g < MPCMP_LIM_GROUPS; g++) {
        excess[g] = A.nan ? NAN : A.ex[g];
        if (channel) channel[g] = (A.nan || A.key[g] == LIM_NO_KEY) ? -1 : (int)(A.key[g] & 0xFu);
    }
    if (ratios) for (int k = 0; k < 4; k++) ratios[k] = A.r[k];
    return MPCMP_OK;
}
