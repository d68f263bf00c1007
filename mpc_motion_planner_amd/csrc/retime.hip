// retime.hip — retiming of finished plans (include/mpcmp_retime.h): per trajectory the time-optimal rate along its own path under the velocity,
// acceleration, torque and tool-speed limits at the points of a grid, the sampler of the retimed plan, and the host statement that needs no
// context.  A translation unit of its own, so that the register-bound QP kernels of solver.hip compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "retime.hpp"
#include "sample_device.hpp"
#include "kinematics_host.hpp"
#include "rnea_host.hpp"

namespace mpcmp {

constexpr int RT_STRIDE = RT_CHUNK + 1;      // doubles between two fields of a record in LDS: lanes that read different fields of one point hit different banks

// the value lane j holds (j wave-uniform)
__device__ __forceinline__ double rt_lane(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}
// minimum / maximum over the wave, in every lane.  Exact, so the order of the butterfly does not matter.
__device__ __forceinline__ double rt_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double rt_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// One workgroup of ONE WAVE per trajectory.  Staged in LDS once: the nodes of the trajectory and the bounds row of the problem, as in k_limits.
// The grid is taken in chunks of 64 points.  For a chunk every lane forms the record of its point (rt_record: three rnea_dir calls and one
// fk_task_velocity per arm, the work k_limits does per sample) and writes it to LDS, 36 doubles per point and arm, so LDS does not grow with n_grid.
// Then the wave walks the chunk point by point: lane r holds row r of the point (28 per arm, then the two next-state rows).  Backward, a lane whose
// row has A > 0 eliminates w against every row with A < 0 (read by v_readlane, skipped wave-uniformly otherwise) and the wave reduces the cuts
// to [lo_k, hi_k]; forward, the lanes reduce the largest w.  The backward pass goes over the chunks from the last to the first and leaves
// (lo_k, hi_k) in prof; the forward pass recomputes the records chunk by chunk, reads the sets back and overwrites them with (t_k, x_k).  Lane l
// writes and reads point 64 c + l of prof (and lane 0 point 64 c + 64, its own of the next chunk), so no lane reads what another lane wrote.
__global__ __launch_bounds__(RT_NT) void k_retime(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int n,
                                                  const mpcmp_bounds *__restrict__ rows, mpcmp_bounds table, const double *__restrict__ sx,
                                                  const double *__restrict__ su, const double *__restrict__ sT, mpcmp_retime_spec sp,
                                                  double *__restrict__ prof, mpcmp_retime *__restrict__ out) {
    __shared__ double nodes[RT_MAX_NODES * 21 * RT_MAX_ARMS];      // x [N][14 narm], then u [N][7 narm]
    __shared__ double bd[58];
    __shared__ double rec[RT_MAX_ARMS * RT_NF * RT_STRIDE];
    const int b = blockIdx.x, lane = threadIdx.x, N = 3 * nseg + 1, nq = 7 * narm;
    double *Xs = nodes, *Us = nodes + 2 * nq * N;
    const double *X = sx + (size_t)b * N * 2 * nq, *U = su + (size_t)b * N * nq;
    const double T = sT[b];
    int bad = !(rt_finite(T) && T > 0.0);
    for (int e = lane; e < 2 * nq * N; e += RT_NT) { Xs[e] = X[e]; bad |= !rt_finite(Xs[e]); }
    for (int e = lane; e < nq * N; e += RT_NT) { Us[e] = U[e]; bad |= !rt_finite(Us[e]); }
    {
        const double *row = reinterpret_cast<const double *>(rows + b), *tab = reinterpret_cast<const double *>(&table);
        for (int e = lane; e < 58; e += RT_NT) bd[e] = rows ? row[e] : tab[e];
    }
    __syncthreads();
    double *pf = prof + (size_t)b * (n + 1) * 2;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    int status = __any(bad) ? MPCMP_RT_NAN : 0, k_fail = -1;

    const double h = 0.5 / T, delta = 1.0 / n, rmax2 = sp.rate_max * sp.rate_max;
    const int nch = n / RT_CHUNK + 1, nrows = RT_ROWS_ARM * narm;
    const int my_arm = lane / RT_ROWS_ARM, my_rr = lane % RT_ROWS_ARM;
    double lo1 = 0.0, hi1 = 0.0, x = 0.0, t = 0.0, xmin = INFINITY;
    int pin0 = 0, kmin = 0, nslow = 0;
    for (int it = 0; it < 2 * nch && !status; it++) {
        const bool fwd = it >= nch;
        const int c = fwd ? it - nch : nch - 1 - it, k = c * RT_CHUNK + lane, npt = min(RT_CHUNK, n + 1 - c * RT_CHUNK);
        if (k <= n) {
            double Lg[4];
            const int s = lagrange_segment(nseg, (double)k / n, Lg);
            for (int a = 0; a < narm; a++) {
                const mpcmp_model *M = mdl + (size_t)b * mstride + a;
                double q[7], v[7], ac[7], sc[14], tc[7], t1[7], t2[7];
                const double zero[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                interp_joints(Xs + 7 * a, Xs + nq + 7 * a, 2 * nq, Us + 7 * a, nq, s, Lg, q, v, ac, sc);
                rnea_dir<false>(M, sc, zero, zero, 0, 0, tc, nullptr);
                rnea_dir<false>(M, sc, v, ac, 0, 0, t1, nullptr);
                rnea_dir<false>(M, sc, zero, v, 0, 0, t2, nullptr);
                V3 pt, vl, va;
                fk_task_velocity(M, sc, v, &pt, &vl, &va);
                rt_record(bd, sp, v, ac, tc, t1, t2, sqrt(vl.x * vl.x + vl.y * vl.y + vl.z * vl.z), sqrt(va.x * va.x + va.y * va.y + va.z * va.z),
                          rec + a * RT_NF * RT_STRIDE + lane, RT_STRIDE);
            }
        }
        __syncthreads();
        double mine0 = qnan, mine1 = qnan;          // what this lane writes to its point of prof: (lo, hi) backward, (t, x) forward
        double setlo = 0.0, sethi = 0.0, nlo = 0.0, nhi = 0.0;
        if (fwd) {
            if (lane < npt) { setlo = pf[2 * k]; sethi = pf[2 * k + 1]; }
            const int kn = (c + 1) * RT_CHUNK;
            if (lane == 0 && kn <= n) { nlo = pf[2 * kn]; nhi = pf[2 * kn + 1]; }
            nlo = rt_lane(nlo, 0); nhi = rt_lane(nhi, 0);
        }
        for (int i = 0; i < npt && !status; i++) {
            const int l = fwd ? i : npt - 1 - i, kk = c * RT_CHUNK + l;
            double A = 0.0, B = 0.0, C = -1.0;
            if (lane < nrows) rt_row(rec + my_arm * RT_NF * RT_STRIDE + l, RT_STRIDE, bd, h, sp.groups, my_rr, A, B, C);
            if (fwd) {
                if (kk == 0) { x = pin0 ? 1.0 : rt_lane(sethi, 0); t = 0.0; }
                if (x < xmin) { xmin = x; kmin = kk; }
                if (x < rmax2) nslow++;
                if (lane == l) { mine0 = t; mine1 = x; }
                if (kk < n) {
                    lo1 = l + 1 < RT_CHUNK ? rt_lane(setlo, l + 1) : nlo;
                    hi1 = l + 1 < RT_CHUNK ? rt_lane(sethi, l + 1) : nhi;
                    if (lane == nrows) { A = delta; B = 1.0; C = -hi1; }
                    const double w = rt_wave_min(A > 0.0 ? rt_w_max(A, B, C, x) : INFINITY);
                    const double x1 = fmin(fmax(x + delta * w, lo1), hi1);
                    t += rt_dt(T, delta, x, x1);
                    x = x1;
                }
                continue;
            }
            double cap = rec[RT_CAP * RT_STRIDE + l];
            if (narm == 2) cap = fmin(cap, rec[(RT_NF + RT_CAP) * RT_STRIDE + l]);
            int moving = 0;
            if (kk == 0 || kk == n) moving = __any(lane < nq && rec[((lane / 7) * RT_NF + RT_V + lane % 7) * RT_STRIDE + l] != 0.0);
            RtSet S = {0.0, INFINITY, 0};
            if (kk < n) {
                if (lane == nrows) { A = delta; B = 1.0; C = -hi1; }
                if (lane == nrows + 1) { A = -delta; B = -1.0; C = lo1; }
            }
            if (A == 0.0) rt_cut_x(S, B, C);
            if (kk < n) {
                for (int j = 0; j < nrows + 2; j++) {
                    const double Aj = rt_lane(A, j);
                    if (!(Aj < 0.0)) continue;
                    const double Bj = rt_lane(B, j), Cj = rt_lane(C, j);
                    if (A > 0.0) rt_cut_pair(S, A, B, C, Aj, Bj, Cj);
                }
            }
            double lo = rt_wave_max(S.lo), hi = fmin(rt_wave_min(S.hi), cap);
            bool fail = __any(S.empty) || !(lo <= hi) || hi == 0.0;
            if (moving) {                           // a pinned end
                fail = fail || !(lo <= 1.0 && 1.0 <= hi);
                if (kk == n) lo = hi = 1.0;
                else pin0 = 1;
            }
            if (fail) { status = MPCMP_RT_INFEASIBLE; k_fail = kk; break; }
            lo1 = lo; hi1 = hi;
            if (lane == l) { mine0 = lo; mine1 = hi; }
        }
        if (!status && lane < npt) { pf[2 * k] = mine0; pf[2 * k + 1] = mine1; }
        __syncthreads();
    }
    if (!status && !rt_finite(t)) status = MPCMP_RT_INFEASIBLE;
    if (status) for (int k = lane; k <= n; k += RT_NT) { pf[2 * k] = qnan; pf[2 * k + 1] = qnan; }
    if (lane == 0) {
        mpcmp_retime r = rt_failed(status, k_fail);
        if (!status) { r.T_new = t; r.rate_min = sqrt(xmin); r.s_slowest = (double)kmin / n; r.n_slowed = nslow; }
        out[b] = r;
    }
}

// One thread per (problem, sample): the interval of the physical time by bisection on the t_k of the profile, then the retimed-sample rule.
__global__ __launch_bounds__(128) void k_sample_retimed(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int B, int n, int n_pts,
                                                        const double *__restrict__ sx, const double *__restrict__ su, const double *__restrict__ sT,
                                                        const double *__restrict__ prof, double *__restrict__ out) {
    const long idx = (long)blockIdx.x * 128 + threadIdx.x;
    if (idx >= (long)B * (n_pts + 1)) return;
    const int b = (int)(idx / (n_pts + 1)), i = (int)(idx % (n_pts + 1)), N = 3 * nseg + 1, nq = 7 * narm, W = 1 + 28 * narm;
    const double *pf = prof + (size_t)b * (n + 1) * 2;
    double *o = out + (size_t)idx * W;
    const double Tn = pf[2 * n], T = sT[b];
    if (!rt_finite(Tn)) {
        for (int e = 0; e < W; e++) o[e] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const double t = ((double)i / n_pts) * Tn;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pf[2 * mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int k = lo;
    const double tk = pf[2 * k], xk = pf[2 * k + 1], x1 = pf[2 * k + 3], lk = sqrt(xk), w = (x1 - xk) * n, h = 0.5 / T;
    double lam = lk + w * (t - tk) * h, s = (double)k / n + (t - tk) * (lk + lam) * h;
    if (i == n_pts) { lam = sqrt(x1); s = 1.0; }
    s = fmin(fmax(s, 0.0), 1.0);
    const double xs = lam * lam;
    const double *X = sx + (size_t)b * N * 2 * nq, *U = su + (size_t)b * N * nq;
    double Lg[4];
    const int seg = lagrange_segment(nseg, s, Lg);
    o[0] = t;
    for (int a = 0; a < narm; a++) {
        double q[7], v[7], ac[7], sc[14], qd[7], qdd[7], tau[7];
        interp_joints(X + 7 * a, X + nq + 7 * a, 2 * nq, U + 7 * a, nq, seg, Lg, q, v, ac, sc);
#pragma unroll
        for (int r = 0; r < 7; r++) { qd[r] = lam * v[r]; qdd[r] = xs * ac[r] + w * h * v[r]; }
        rnea_dir<false>(mdl + (size_t)b * mstride + a, sc, qd, qdd, 0, 0, tau, nullptr);
#pragma unroll
        for (int r = 0; r < 7; r++) { o[1 + 28 * a + r] = q[r]; o[8 + 28 * a + r] = qd[r]; o[15 + 28 * a + r] = qdd[r]; o[22 + 28 * a + r] = tau[r]; }
    }
}

hipError_t retime_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int n_grid, const mpcmp_bounds *rows, const mpcmp_bounds &table,
                         const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_retime_spec &spec, double *d_prof, mpcmp_retime *d_out,
                         hipStream_t st) {
    if (narm < 1 || narm > RT_MAX_ARMS || nseg < 1 || 3 * nseg + 1 > RT_MAX_NODES || n_grid < 1 || n_grid > RT_MAX_GRID || B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_retime, dim3(B), dim3(RT_NT), 0, st, mdl, mstride, narm, nseg, n_grid, rows, table, d_sx, d_su, d_sT, spec, d_prof, d_out);
    return hipGetLastError();
}

hipError_t sample_retimed_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int n_grid, int n_pts, const double *d_sx,
                                 const double *d_su, const double *d_sT, const double *d_prof, double *d_out, hipStream_t st) {
    if (narm < 1 || narm > RT_MAX_ARMS || nseg < 1 || 3 * nseg + 1 > RT_MAX_NODES || n_grid < 1 || n_grid > RT_MAX_GRID || n_pts < 1 || B < 1) return hipErrorInvalidValue;
    const long total = (long)B * (n_pts + 1);
    hipLaunchKernelGGL(k_sample_retimed, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, st, mdl, mstride, narm, nseg, B, n_grid, n_pts, d_sx, d_su,
                       d_sT, d_prof, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host statement (no GPU): the records from plain host C++, then the row, pair and clock arithmetic of retime.hpp ----
namespace {
// lagrange_segment and interp_joints (sample_device.hpp) for one arm on the host
int lagrange_host(int nseg, double t, double *Lg) {
    const double xi[4] = {-1.0, -0.5, 0.5, 1.0};
    int s = (int)std::floor(t * nseg);
    if (s >= nseg) s = nseg - 1;
    if (s < 0) s = 0;
    const double xx = 2.0 * (t * nseg - s) - 1.0;
    for (int j = 0; j < 4; j++) {
        double v = 1.0;
        for (int k = 0; k < 4; k++) if (k != j) v *= (xx - xi[k]) / (xi[j] - xi[k]);
        Lg[j] = v;
    }
    return s;
}
}  // namespace

extern "C" int mpcmp_retime_one(const mpcmp_model *models, int narm, int num_seg, const mpcmp_bounds *row, const mpcmp_retime_spec *spec,
                                const double *x, const double *u, double T, int n_grid, double *prof, mpcmp_retime *out) {
    if (!models || narm < 1 || narm > RT_MAX_ARMS || num_seg < 1 || 3 * num_seg + 1 > RT_MAX_NODES || !row || !x || !u || n_grid < 1 ||
        n_grid > RT_MAX_GRID || !prof || !out) return MPCMP_EINVAL;
    const mpcmp_retime_spec sp = spec ? *spec : rt_default_spec();
    if (!rt_spec_ok(sp)) return MPCMP_EINVAL;
    const int n = n_grid, N = 3 * num_seg + 1, nq = 7 * narm, nrows = RT_ROWS_ARM * narm;
    const double *bd = reinterpret_cast<const double *>(row);
    auto fill_nan = [&]() { for (int e = 0; e < 2 * (n + 1); e++) prof[e] = NAN; };
    bool bad = !(std::isfinite(T) && T > 0.0);
    for (int e = 0; e < 2 * nq * N; e++) bad = bad || !std::isfinite(x[e]);
    for (int e = 0; e < nq * N; e++) bad = bad || !std::isfinite(u[e]);
    if (bad) { fill_nan(); *out = rt_failed(MPCMP_RT_NAN, -1); return MPCMP_OK; }

    std::vector<double> rec((size_t)(n + 1) * narm * RT_NF), Klo(n + 1), Khi(n + 1);
    for (int k = 0; k <= n; k++) {
        double Lg[4];
        const int s = lagrange_host(num_seg, (double)k / n, Lg);
        for (int a = 0; a < narm; a++) {
            double q[7], v[7], ac[7], tc[7], t1[7], t2[7], J[42], p[3], R[9], tw[6];
            const double zero[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int r = 0; r < 7; r++) {
                q[r] = v[r] = ac[r] = 0.0;
                for (int j = 0; j < 4; j++) {
                    q[r] += Lg[j] * x[2 * nq * (3 * s + j) + 7 * a + r];
                    v[r] += Lg[j] * x[2 * nq * (3 * s + j) + nq + 7 * a + r];
                    ac[r] += Lg[j] * u[nq * (3 * s + j) + 7 * a + r];
                }
            }
            mpcmp_host::rnea_host(models[a], q, zero, zero, tc);
            mpcmp_host::rnea_host(models[a], q, v, ac, t1);
            mpcmp_host::rnea_host(models[a], q, zero, v, t2);
            mpcmp_host::tool_jacobian(models[a], q, J, p, R);
            for (int r = 0; r < 6; r++) { tw[r] = 0.0; for (int j = 0; j < 7; j++) tw[r] += J[7 * r + j] * v[j]; }
            rt_record(bd, sp, v, ac, tc, t1, t2, std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]),
                      std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]), &rec[((size_t)k * narm + a) * RT_NF], 1);
        }
    }
    const double h = 0.5 / T, delta = 1.0 / n, rmax2 = sp.rate_max * sp.rate_max;
    double A[RT_ROWS_ARM * RT_MAX_ARMS + 2], Bc[RT_ROWS_ARM * RT_MAX_ARMS + 2], Cc[RT_ROWS_ARM * RT_MAX_ARMS + 2];
    auto point_rows = [&](int k) { for (int r = 0; r < nrows; r++) rt_row(&rec[((size_t)k * narm + r / RT_ROWS_ARM) * RT_NF], 1, bd, h, sp.groups, r % RT_ROWS_ARM, A[r], Bc[r], Cc[r]); };
    auto moving = [&](int k) { for (int a = 0; a < narm; a++) for (int j = 0; j < 7; j++) if (rec[((size_t)k * narm + a) * RT_NF + RT_V + j] != 0.0) return true; return false; };
    auto cap_of = [&](int k) { double c = INFINITY; for (int a = 0; a < narm; a++) c = fmin(c, rec[((size_t)k * narm + a) * RT_NF + RT_CAP]); return c; };
    const bool pin0 = moving(0), pinn = moving(n);
    // backward
    for (int k = n; k >= 0; k--) {
        point_rows(k);
        int m = nrows;
        if (k < n) { A[m] = delta; Bc[m] = 1.0; Cc[m] = -Khi[k + 1]; m++; A[m] = -delta; Bc[m] = -1.0; Cc[m] = Klo[k + 1]; m++; }
        RtSet S = {0.0, INFINITY, 0};
        for (int i = 0; i < m; i++) {
            if (A[i] == 0.0) rt_cut_x(S, Bc[i], Cc[i]);
            if (k < n && A[i] > 0.0) for (int j = 0; j < m; j++) if (A[j] < 0.0) rt_cut_pair(S, A[i], Bc[i], Cc[i], A[j], Bc[j], Cc[j]);
        }
        double lo = S.lo, hi = fmin(S.hi, cap_of(k));
        bool fail = S.empty || !(lo <= hi) || hi == 0.0;
        if ((k == n && pinn) || (k == 0 && pin0)) {
            fail = fail || !(lo <= 1.0 && 1.0 <= hi);
            if (k == n) lo = hi = 1.0;
        }
        if (fail) { fill_nan(); *out = rt_failed(MPCMP_RT_INFEASIBLE, k); return MPCMP_OK; }
        Klo[k] = lo; Khi[k] = hi;
    }
    // forward
    double xk = pin0 ? 1.0 : Khi[0], t = 0.0, xmin = INFINITY;
    int kmin = 0, nslow = 0;
    for (int k = 0; k <= n; k++) {
        if (xk < xmin) { xmin = xk; kmin = k; }
        if (xk < rmax2) nslow++;
        prof[2 * k] = t; prof[2 * k + 1] = xk;
        if (k == n) break;
        point_rows(k);
        double w = rt_w_max(delta, 1.0, -Khi[k + 1], xk);
        for (int r = 0; r < nrows; r++) if (A[r] > 0.0) w = fmin(w, rt_w_max(A[r], Bc[r], Cc[r], xk));
        const double x1 = fmin(fmax(xk + delta * w, Klo[k + 1]), Khi[k + 1]);
        t += rt_dt(T, delta, xk, x1);
        xk = x1;
    }
    if (!std::isfinite(t)) { fill_nan(); *out = rt_failed(MPCMP_RT_INFEASIBLE, -1); return MPCMP_OK; }
    mpcmp_retime r = rt_failed(0, -1);
    r.T_new = t; r.rate_min = std::sqrt(xmin); r.s_slowest = (double)kmin / n; r.n_slowed = nslow;
    *out = r;
    return MPCMP_OK;
}
