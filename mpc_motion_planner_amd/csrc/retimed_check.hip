// retimed_check.hip — the limit checker of retimed plans and routes (include/mpcmp_retimed_check.h): per plan or route the record of mpcmp_limits.h
// for the motion its rate profile stands for, at the uniform physical times of the retimed samplers; the uniform scaling of a profile; and the host
// statement that needs no context.  A plan is a route of one leg: the plan call runs k_limits_retimed with M = 0.  A translation unit of its own, so
// that k_limits, k_retime, the samplers and the register-bound QP kernels compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "retimed_check.hpp"
#include "sample_device.hpp"
#include "kinematics_host.hpp"
#include "rnea_host.hpp"

namespace mpcmp {

// One sample folded into A: the nodes X [N][2 nq], U [N][nq] (LDS or global), the bounds row bd [58], the models of the slot, the place on the
// profile.  For every arm in turn the Lagrange rule of sample_row at s, the retimed velocity and acceleration, sine / cosine, the RNEA torque with
// the arm's model and one forward-kinematics pass for the tool position and twist; lim_fold_arm compares.
__device__ __forceinline__ void rc_fold_sample(LimAcc &A, const mpcmp_model *__restrict__ Ms, int narm, int nseg, const double *X, const double *U,
                                               const double *bd, const mpcmp_limits_spec &sp, int ip, const RcPlace &pl) {
    const int nq = 7 * narm;
    const double xs = pl.lam * pl.lam;
    double Lg[4];
    const int seg = lagrange_segment(nseg, pl.s, Lg);
    bool over = false;
    for (int a = 0; a < narm; a++) {
        double q[7], v[7], ac[7], qd[7], qdd[7], tau[7], sc[14];
        interp_joints(X + 7 * a, X + nq + 7 * a, 2 * nq, U + 7 * a, nq, seg, Lg, q, v, ac, sc);
#pragma unroll
        for (int r = 0; r < 7; r++) { qd[r] = pl.lam * v[r]; qdd[r] = xs * ac[r] + pl.wh * v[r]; }
        rnea_dir<false>(Ms + a, sc, qd, qdd, 0, 0, tau, nullptr);
        V3 pt, vl, va;
        fk_task_velocity(Ms + a, sc, qd, &pt, &vl, &va);
        over |= lim_fold_arm(A, bd, sp, ip, a, q, qd, qdd, tau, pt.z, sqrt(vl.x * vl.x + vl.y * vl.y + vl.z * vl.z),
                             sqrt(va.x * va.x + va.y * va.y + va.z * va.z));
    }
    lim_count(A, ip, over);
}

// The workgroup reduction of k_limits: the (excess, key) pairs by lim_better, the maxima of the ratios (exact, so order-free), the sums of the counts
// and the minimum of the first indices; thread 0 writes the record with the times of the retimed clock.  No atomics.
__device__ __forceinline__ void rc_reduce_write(LimAcc &A, int tid, const mpcmp_limits_spec &sp, int n_pts, double Tn, mpcmp_limits *__restrict__ out,
                                                double *__restrict__ Tnew, int b) {
    constexpr int NW = LIM_NT / 64;
    __shared__ double red_e[NW][MPCMP_LIM_GROUPS], red_r[NW][4];
    __shared__ unsigned red_k[NW][MPCMP_LIM_GROUPS];
    __shared__ int red_i[NW][3];
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
        out[b] = rc_record(A, sp, n_pts, Tn);
        if (Tnew) Tnew[b] = Tn;
    }
}

// the record of a failed profile (a t_n that is not finite), written by thread 0
__device__ __forceinline__ void rc_write_failed(const mpcmp_limits_spec &sp, int n_pts, mpcmp_limits *__restrict__ out, double *__restrict__ Tnew, int b) {
    LimAcc A;
    lim_init(A);
    A.nan = 1;
    out[b] = rc_record(A, sp, n_pts, INFINITY);
    if (Tnew) Tnew[b] = INFINITY;
}

// One workgroup per route of M + 1 legs (a plan: M = 0), the shape of k_limits.  Every thread forms the retimed leg durations D_m = the last t of
// each leg's profile and their sum T_new sequentially, as k_sample_retimed does.  Then the legs in turn: the nodes (x and u, at most 25 x 42 doubles)
// and the bounds row of the leg slot are staged in LDS, and every thread takes those of its samples (strided, so increasing in time) that the
// sampler's rule places in this leg: with E_m the sequential prefix sums, the first leg with t < E_m, leg M for what is left and for sample n_pts.
// Per sample a bisection on the t_k of the leg's profile in global memory (at most 12 steps over at most 64 KB per leg, which stay in L2), the
// retimed-sample rule, and rc_fold_sample.  Nothing of a sample is stored: a thread keeps its LimAcc in registers over all its samples, and one
// workgroup reduction ends the kernel.  Static LDS only, and none of it grows with n_pts, n_grid or M.  The key stays sample << 4 | channel: ties go
// to the lowest sample of the route clock.  ONE_LEG: the same text compiled with M == 0 known, which the launcher takes for M = 0: without it a plan
// call measured 1.8 % slower than the plan kernel this one replaces ("One kernel set for plans and routes").
template <bool ONE_LEG>
__global__ __launch_bounds__(LIM_NT) void k_limits_retimed(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int n, int legs_m,
                                                           int n_pts, const mpcmp_bounds *__restrict__ rows, mpcmp_bounds table,
                                                           const double *__restrict__ sx, const double *__restrict__ su,
                                                           const double *__restrict__ sT, const double *__restrict__ prof,
                                                           mpcmp_limits_spec sp, mpcmp_limits *__restrict__ out, double *__restrict__ Tnew) {
    __shared__ double nodes[LIM_MAX_NODES * 21 * LIM_MAX_ARMS];      // x [N][14 narm], then u [N][7 narm] of the leg in hand
    __shared__ double bd[58];
    const int M = ONE_LEG ? 0 : legs_m;
    const int b = blockIdx.x, tid = threadIdx.x, N = 3 * nseg + 1, nq = 7 * narm, nl = M + 1;
    const size_t l0 = (size_t)b * nl, ps = (size_t)(n + 1) * 2;
    double Tn = 0.0;
    bool finite = true, Tok = true;
    for (int m = 0; m < nl; m++) {
        const double D = prof[(l0 + m) * ps + 2 * n];
        Tn = m ? Tn + D : D;
        finite = finite && lim_finite(D);
        Tok = Tok && lim_finite(sT[l0 + m]);
    }
    if (!finite) {                               // (the same for every thread of the workgroup)
        if (tid == 0) rc_write_failed(sp, n_pts, out, Tnew, b);
        return;
    }
    double *Xs = nodes, *Us = nodes + 2 * nq * N;
    LimAcc A;
    lim_init(A);
    if (!Tok) A.nan = 1;
    int ip = tid;
    double Ep = 0.0;
    for (int leg = 0; leg < nl; leg++) {
        const size_t ls = l0 + leg;
        const double *pf = prof + ls * ps;
        const double D = pf[2 * n], E = Ep + D, h = 0.5 / sT[ls];
        const double *X = sx + ls * N * 2 * nq, *U = su + ls * N * nq;
        __syncthreads();                         // (the leg before is done with the LDS)
        for (int e = tid; e < 2 * nq * N; e += LIM_NT) Xs[e] = X[e];
        for (int e = tid; e < nq * N; e += LIM_NT) Us[e] = U[e];
        {
            const double *row = reinterpret_cast<const double *>(rows + ls), *tab = reinterpret_cast<const double *>(&table);
            for (int e = tid; e < 58; e += LIM_NT) bd[e] = rows ? row[e] : tab[e];
        }
        __syncthreads();
        for (; ip <= n_pts; ip += LIM_NT) {
            const double t = ((double)ip / n_pts) * Tn;
            if (leg < M && (ip == n_pts || !(t < E))) break;
            const RcPlace pl = rc_place(pf, n, fmin(fmax(t - Ep, 0.0), D), h, ip == n_pts);
            rc_fold_sample(A, mdl + ls * mstride, narm, nseg, Xs, Us, bd, sp, ip, pl);
        }
        Ep = E;
    }
    rc_reduce_write(A, tid, sp, n_pts, Tn, out, Tnew, b);
}

// One thread per (slot, grid point): t_k *= f, x_k /= f^2; a factor that is not finite or <= 0 makes the slot's profile NaN
__global__ __launch_bounds__(256) void k_profile_scale(int L, int n, const double *__restrict__ factor, double *__restrict__ prof) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)L * (n + 1)) return;
    const double f = factor[idx / (n + 1)];
    double *p = prof + 2 * idx;
    if (!(lim_finite(f) && f > 0.0)) { p[0] = NAN; p[1] = NAN; return; }
    p[0] = p[0] * f;
    p[1] = p[1] / (f * f);
}

static bool rc_shape_ok(int narm, int nseg, int B, int M, int n_grid, int n_pts) {
    return narm >= 1 && narm <= LIM_MAX_ARMS && nseg >= 1 && 3 * nseg + 1 <= LIM_MAX_NODES && n_grid >= 1 && n_grid <= RT_MAX_GRID && n_pts >= 1 &&
           n_pts <= LIM_MAX_PTS && B >= 1 && M >= 0;
}

hipError_t limits_retimed_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, int n_pts,
                                 const mpcmp_bounds *rows, const mpcmp_bounds &table, const double *d_sx, const double *d_su, const double *d_sT,
                                 const double *d_prof, const mpcmp_limits_spec &spec, mpcmp_limits *d_out, double *d_Tnew, hipStream_t st) {
    if (!rc_shape_ok(narm, nseg, B, M, n_grid, n_pts)) return hipErrorInvalidValue;
    const auto kernel = M == 0 ? k_limits_retimed<true> : k_limits_retimed<false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(LIM_NT), 0, st, mdl, mstride, narm, nseg, n_grid, M, n_pts, rows, table, d_sx, d_su, d_sT, d_prof, spec,
                       d_out, d_Tnew);
    return hipGetLastError();
}

hipError_t profile_scale_launch(int L, int n_grid, const double *d_factor, double *d_prof, hipStream_t st) {
    if (L < 1 || n_grid < 1 || n_grid > RT_MAX_GRID) return hipErrorInvalidValue;
    const long total = (long)L * (n_grid + 1);
    hipLaunchKernelGGL(k_profile_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, L, n_grid, d_factor, d_prof);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host statement (no GPU): the samples from plain host C++, then the place, fold and record arithmetic of retimed_check.hpp / limits.hpp ----
extern "C" int mpcmp_limits_retimed_one(const mpcmp_model *models, int narm, int num_seg, int n_legs, const mpcmp_bounds *rows,
                                        const mpcmp_limits_spec *spec, const double *x, const double *u, const double *T, int n_grid,
                                        const double *prof, int n_pts, mpcmp_limits *out, double *T_new) {
    if (!models || narm < 1 || narm > LIM_MAX_ARMS || num_seg < 1 || 3 * num_seg + 1 > LIM_MAX_NODES || n_legs < 1 || !rows || !x || !u || !T ||
        n_grid < 1 || n_grid > RT_MAX_GRID || !prof || n_pts < 1 || n_pts > LIM_MAX_PTS || !out) return MPCMP_EINVAL;
    const mpcmp_limits_spec sp = spec ? *spec : lim_default_spec();
    if (!lim_spec_ok(sp)) return MPCMP_EINVAL;
    const int n = n_grid, N = 3 * num_seg + 1, nq = 7 * narm, nl = n_legs;
    const size_t ps = (size_t)(n + 1) * 2;
    LimAcc A;
    lim_init(A);
    double Tn = 0.0;
    bool finite = true;
    for (int m = 0; m < nl; m++) {
        const double D = prof[m * ps + 2 * n];
        Tn = m ? Tn + D : D;
        finite = finite && lim_finite(D);
        if (!lim_finite(T[m])) A.nan = 1;
    }
    if (!finite) {
        A.nan = 1;
        *out = rc_record(A, sp, n_pts, INFINITY);
        if (T_new) *T_new = INFINITY;
        return MPCMP_OK;
    }
    for (int ip = 0; ip <= n_pts; ip++) {
        const double t = ((double)ip / n_pts) * Tn;
        double Ep = 0.0;
        int leg = 0;
        for (;;) {
            const double E = Ep + prof[leg * ps + 2 * n];
            if (t < E || leg == nl - 1) break;
            Ep = E; leg++;
        }
        if (ip == n_pts) leg = nl - 1;
        const double *pf = prof + leg * ps, *xm = x + (size_t)leg * N * 2 * nq, *um = u + (size_t)leg * N * nq;
        const double tl = fmin(fmax(t - Ep, 0.0), pf[2 * n]);
        const RcPlace pl = rc_place(pf, n, tl, 0.5 / T[leg], ip == n_pts);
        const double xs = pl.lam * pl.lam;
        double Lg[4];
        const int s = mpcmp_plan::lagrange_segment(num_seg, pl.s, Lg);
        bool over = false;
        for (int a = 0; a < narm; a++) {
            double q[7], v[7], ac[7], qd[7], qdd[7], tau[7], J[42], p[3], R[9], tw[6];
            mpcmp_plan::interp_qva(xm + 7 * a, xm + nq + 7 * a, 2 * nq, um + 7 * a, nq, s, Lg, q, v, ac);
            for (int r = 0; r < 7; r++) { qd[r] = pl.lam * v[r]; qdd[r] = xs * ac[r] + pl.wh * v[r]; }
            mpcmp_host::rnea_host(models[a], q, qd, qdd, tau);
            mpcmp_host::tool_jacobian(models[a], q, J, p, R);
            for (int r = 0; r < 6; r++) { tw[r] = 0.0; for (int j = 0; j < 7; j++) tw[r] += J[7 * r + j] * qd[j]; }
            over |= lim_fold_arm(A, reinterpret_cast<const double *>(rows + leg), sp, ip, a, q, qd, qdd, tau, p[2],
                                 std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]), std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]));
        }
        lim_count(A, ip, over);
    }
    *out = rc_record(A, sp, n_pts, Tn);
    if (T_new) *T_new = Tn;
    return MPCMP_OK;
}
