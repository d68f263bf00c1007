// route.hip — via-point routes (include/mpcmp.h, "via-point routes"): the leg builder with the chord rule, the join of the legs' records into one
// record per route, the sampling of a route on a uniform clock across its junctions, and the host helpers that need no context.
// A translation unit of its own, so that the register-bound QP kernels of solver.hip compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "route.hpp"
#include "sample_device.hpp"

namespace mpcmp {

// point i = 0 .. M + 1 of route b: q(x0), the vias, q(xf); each 7 narm contiguous doubles
__device__ __forceinline__ const double *route_point(int i, int b, int M, int nq, const double *x0, const double *via, const double *xf) {
    if (i == 0) return x0 + (size_t)b * 2 * nq;
    if (i == M + 1) return xf + (size_t)b * 2 * nq;
    return via + ((size_t)b * M + (i - 1)) * nq;
}

// One thread per leg slot l = b (M + 1) + m: the leg runs from (P_m, V_m) to (P_m+1, V_m+1).  A via's velocity is formed twice, by the leg that ends
// there and by the leg that starts there, from the same inputs by the same function: the two agree bit for bit.  The limits of via i are those of
// the leg slot that STARTS there, b (M + 1) + i; the thread of that leg writes via_qd_out.
__global__ __launch_bounds__(128) void k_route_legs(int B, int M, int narm, const double *__restrict__ x0, const double *__restrict__ via,
                                                    const double *__restrict__ via_qd, const double *__restrict__ speed, const double *__restrict__ xf,
                                                    const mpcmp_bounds *__restrict__ rows, mpcmp_bounds cfg_row, double *__restrict__ leg_x0,
                                                    double *__restrict__ leg_xf, double *__restrict__ via_qd_out) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= B * (M + 1)) return;
    const int b = l / (M + 1), m = l % (M + 1), nq = 7 * narm;
    const double sp = speed ? speed[b] : 1.0;
    for (int end = 0; end < 2; end++) {
        const int i = m + end;                             // the point this end of the leg lies at
        double *o = (end ? leg_xf : leg_x0) + (size_t)l * 2 * nq;
        const double *P = route_point(i, b, M, nq, x0, via, xf);
        double V[14];
        if (i == 0 || i == M + 1) { for (int j = 0; j < nq; j++) V[j] = P[nq + j]; }
        else if (via_qd) { for (int j = 0; j < nq; j++) V[j] = via_qd[((size_t)b * M + (i - 1)) * nq + j]; }
        else
            route_via_velocity(route_point(i - 1, b, M, nq, x0, via, xf), P, route_point(i + 1, b, M, nq, x0, via, xf),
                               rows ? rows + (size_t)b * (M + 1) + i : &cfg_row, narm, sp, V);
        for (int j = 0; j < nq; j++) { o[j] = P[j]; o[nq + j] = V[j]; }
        if (!end && m > 0 && via_qd_out)
            for (int j = 0; j < nq; j++) via_qd_out[((size_t)b * M + (m - 1)) * nq + j] = V[j];
    }
}

// one thread per route: every sum, maximum and tie runs sequentially in leg order (route_join_one)
__global__ __launch_bounds__(64) void k_route_join(int B, int M, int N, int narm, const double *__restrict__ sx, const double *__restrict__ su,
                                                   const double *__restrict__ sT, const mpcmp_info *__restrict__ info,
                                                   const mpcmp_clearance *__restrict__ clr, double *__restrict__ rT, mpcmp_info *__restrict__ rinfo,
                                                   mpcmp_route_seam *__restrict__ seam, mpcmp_clearance *__restrict__ rclr) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int nl = M + 1, nx = 14 * narm, nu = 7 * narm;
    const size_t l0 = (size_t)b * nl;
    route_join_one(nl, N, nx, nu, sx + l0 * N * nx, su + l0 * N * nu, sT + l0, info + l0, clr ? clr + l0 : nullptr, rT + b, rinfo + b, seam + b,
                   rclr ? rclr + b : nullptr);
}

// one thread per (route, sample): the route time, its leg and normalised time (route_locate), then the row k_sample gives for that leg there
// (sample_row), with the model of the leg slot.  A route with a leg T that is no finite number gets NaN rows.
__global__ __launch_bounds__(128) void k_sample_route(const mpcmp_model *mdl, int mstride, int nseg, int B, int M, int n_pts, const double *sx,
                                                      const double *su, const double *sT, double *out) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * (n_pts + 1);
    if (gid >= total) return;
    const int b = (int)(gid / (n_pts + 1)), ip = (int)(gid % (n_pts + 1)), nl = M + 1, N = 3 * nseg + 1;
    const double *T = sT + (size_t)b * nl;
    double *o = out + (size_t)gid * 29;
    double R = 0.0;
    bool finite = true;
    for (int m = 0; m < nl; m++) { R += T[m]; finite = finite && isfinite(T[m]); }
    if (!finite) {
        for (int c = 0; c < 29; c++) o[c] = route_nan();
        return;
    }
    const double t = (double)ip / n_pts * R;
    int leg;
    double tau;
    route_locate(nl, T, t, &leg, &tau);
    if (ip == n_pts) { leg = M; tau = 1.0; }
    const size_t l = (size_t)b * nl + leg;
    sample_row(mdl + l * mstride, nseg, sx + l * 14 * N, su + l * 7 * N, tau, o);
    o[0] = t;
}

hipError_t route_legs_launch(int B, int M, int narm, const double *x0, const double *via, const double *via_qd, const double *speed, const double *xf,
                             const mpcmp_bounds *rows, const mpcmp_bounds &cfg_row, double *leg_x0, double *leg_xf, double *via_qd_out, hipStream_t st) {
    const int L = B * (M + 1);
    hipLaunchKernelGGL(k_route_legs, dim3((L + 127) / 128), dim3(128), 0, st, B, M, narm, x0, via, via_qd, speed, xf, rows, cfg_row, leg_x0, leg_xf,
                       via_qd_out);
    return hipGetLastError();
}

hipError_t route_join_launch(int B, int M, int N, int narm, const double *sx, const double *su, const double *sT, const mpcmp_info *info,
                             const mpcmp_clearance *clr, double *rT, mpcmp_info *rinfo, mpcmp_route_seam *seam, mpcmp_clearance *rclr, hipStream_t st) {
    hipLaunchKernelGGL(k_route_join, dim3((B + 63) / 64), dim3(64), 0, st, B, M, N, narm, sx, su, sT, info, clr, rT, rinfo, seam, rclr);
    return hipGetLastError();
}

hipError_t route_sample_launch(const mpcmp_model *mdl, int mstride, int nseg, int B, int M, int n_pts, const double *sx, const double *su, const double *sT,
                               double *out, hipStream_t st) {
    const long total = (long)B * (n_pts + 1);
    hipLaunchKernelGGL(k_sample_route, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, st, mdl, mstride, nseg, B, M, n_pts, sx, su, sT, out);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host helpers (no GPU): the functions the kernels run ----
extern "C" int mpcmp_route_via_velocity(const double *p_prev, const double *p_via, const double *p_next, const mpcmp_bounds *row, int narm, double speed,
                                        double *v) {
    if (!p_prev || !p_via || !p_next || !row || !v || narm < 1 || narm > 2 || !(speed >= 0.0 && speed <= 1.0)) return MPCMP_EINVAL;
    for (int j = 0; j < 7 * narm; j++)
        if (!std::isfinite(p_prev[j]) || !std::isfinite(p_via[j]) || !std::isfinite(p_next[j])) return MPCMP_EINVAL;
    route_via_velocity(p_prev, p_via, p_next, row, narm, speed, v);
    return MPCMP_OK;
}

extern "C" int mpcmp_route_locate(int n_legs, const double *leg_T, double t, int *leg, double *tau) {
    if (n_legs < 1 || !leg_T || !leg || !tau || t != t) return MPCMP_EINVAL;
    route_locate(n_legs, leg_T, t, leg, tau);
    return MPCMP_OK;
}
