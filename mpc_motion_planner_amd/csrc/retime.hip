// retime.hip — retiming of finished plans and of whole via-point routes (include/mpcmp_retime.h, include/mpcmp_route_retime.h): per route ONE
// time-optimal rate profile along its own path, across its junctions, under the velocity, acceleration, torque and tool-speed limits at the points
// of a grid; the sampler of the retimed route on one clock; and the host statements that need no context.  A plan is a route of one leg: the plan
// calls run the same kernels with M = 0.  A translation unit of its own, so that the register-bound QP kernels of solver.hip compile exactly as before.
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

// One workgroup of ONE WAVE per ROUTE of M + 1 legs (a plan: M = 0).  The wave takes the legs one after the other, backward from the last leg to the
// first and then forward from the first to the last.  Per leg it stages that leg's nodes and bound row in LDS, as k_limits does (the same buffers for
// every leg, so LDS grows neither with n_grid nor with M).  The grid of a leg is taken in chunks of 64 points.  For a chunk every lane forms the
// record of its point (rt_record: three rnea_dir calls and one fk_task_velocity per arm, the work k_limits does per sample) and writes it to LDS, 36
// doubles per point and arm.  Then the wave walks the chunk point by point: lane r holds row r of the point (28 per arm, then the two next-state
// rows).  Backward, a lane whose row has A > 0 eliminates w against every row with A < 0 (read by v_readlane, skipped wave-uniformly otherwise) and
// the wave reduces the cuts to [lo_k, hi_k]; forward, the lanes reduce the largest w.  The backward pass leaves (lo_k, hi_k) in the caller's prof;
// the forward pass recomputes the records chunk by chunk, reads the sets back and overwrites them with (t_k, x_k).  What crosses a junction travels
// in registers: backward (lo1, hi1) = K_0 of the later leg, which the last point of the earlier leg is intersected with; forward x, which the later
// leg starts from.  Lane l reads and writes point 64 c + l of a leg (and lane 0 point 64 c + 64, its own of the next chunk), so no lane reads what
// another lane wrote.  No global workspace, no atomics.  Lane 0 writes the record: to rout, or without its leg fields to pout.
__global__ __launch_bounds__(RT_NT) void k_retime(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int n, int M,
                                                  const mpcmp_bounds *__restrict__ rows, mpcmp_bounds table, const double *__restrict__ sx,
                                                  const double *__restrict__ su, const double *__restrict__ sT, mpcmp_retime_spec sp,
                                                  double *__restrict__ prof, double *__restrict__ legT, mpcmp_retime *__restrict__ pout,
                                                  mpcmp_route_retime *__restrict__ rout) {
    __shared__ double nodes[RT_MAX_NODES * 21 * RT_MAX_ARMS];      // x [N][14 narm], then u [N][7 narm] of the leg at hand
    __shared__ double bd[58];
    __shared__ double rec[RT_MAX_ARMS * RT_NF * RT_STRIDE];
    const int b = blockIdx.x, lane = threadIdx.x, N = 3 * nseg + 1, nq = 7 * narm, nl = M + 1;
    const size_t l0 = (size_t)b * nl;
    double *Xs = nodes, *Us = nodes + 2 * nq * N;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    int status, leg_fail = -1, k_fail = -1;
    {   // a non-finite value anywhere in the route fails all of it before any pass
        const double *X = sx + l0 * N * 2 * nq, *U = su + l0 * N * nq;
        int bad = 0;
        for (int e = lane; e < nl * 2 * nq * N; e += RT_NT) bad |= !rt_finite(X[e]);
        for (int e = lane; e < nl * nq * N; e += RT_NT) bad |= !rt_finite(U[e]);
        for (int m = lane; m < nl; m += RT_NT) { const double Tm = sT[l0 + m]; bad |= !(rt_finite(Tm) && Tm > 0.0); }
        status = __any(bad) ? MPCMP_RT_NAN : 0;
    }

    const double delta = 1.0 / n, rmax2 = sp.rate_max * sp.rate_max;
    const int nch = n / RT_CHUNK + 1, half = nl * nch, nrows = RT_ROWS_ARM * narm;
    const int my_arm = lane / RT_ROWS_ARM, my_rr = lane % RT_ROWS_ARM;
    double T = 1.0, h = 0.5, lo1 = 0.0, hi1 = 0.0, x = 0.0, t = 0.0, Ttot = 0.0, xmin = INFINITY;
    int pin0 = 0, kmin = 0, legmin = 0, nslow = 0;
    for (int it = 0; it < 2 * half && !status; it++) {
        const bool fwd = it >= half;
        const int j = fwd ? it - half : half - 1 - it, leg = j / nch, c = j % nch;
        const size_t ls = l0 + leg;
        if (c == (fwd ? 0 : nch - 1)) {             // a pass enters this leg: stage it (the iteration before ended with a barrier)
            const double *X = sx + ls * N * 2 * nq, *U = su + ls * N * nq;
            for (int e = lane; e < 2 * nq * N; e += RT_NT) Xs[e] = X[e];
            for (int e = lane; e < nq * N; e += RT_NT) Us[e] = U[e];
            const double *row = reinterpret_cast<const double *>(rows + ls), *tab = reinterpret_cast<const double *>(&table);
            for (int e = lane; e < 58; e += RT_NT) bd[e] = rows ? row[e] : tab[e];
            T = sT[ls]; h = 0.5 / T;
            __syncthreads();
        }
        double *pf = prof + ls * (n + 1) * 2;
        const int k = c * RT_CHUNK + lane, npt = min(RT_CHUNK, n + 1 - c * RT_CHUNK);
        if (k <= n) {
            double Lg[4];
            const int s = lagrange_segment(nseg, (double)k / n, Lg);
            for (int a = 0; a < narm; a++) {
                const mpcmp_model *Mo = mdl + ls * mstride + a;
                double q[7], v[7], ac[7], sc[14], tc[7], t1[7], t2[7];
                const double zero[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                interp_joints(Xs + 7 * a, Xs + nq + 7 * a, 2 * nq, Us + 7 * a, nq, s, Lg, q, v, ac, sc);
                rnea_dir<false>(Mo, sc, zero, zero, 0, 0, tc, nullptr);
                rnea_dir<false>(Mo, sc, v, ac, 0, 0, t1, nullptr);
                rnea_dir<false>(Mo, sc, zero, v, 0, 0, t2, nullptr);
                V3 pt, vl, va;
                fk_task_velocity(Mo, sc, v, &pt, &vl, &va);
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
                if (kk == 0) { if (leg == 0) x = pin0 ? 1.0 : rt_lane(sethi, 0); t = 0.0; }       // a later leg starts from the x the leg before ended with
                if (x < xmin) { xmin = x; kmin = kk; legmin = leg; }
                if ((kk > 0 || leg == 0) && x < rmax2) nslow++;                                    // a junction counts once
                if (lane == l) { mine0 = t; mine1 = x; }
                if (kk < n) {
                    lo1 = l + 1 < RT_CHUNK ? rt_lane(setlo, l + 1) : nlo;
                    hi1 = l + 1 < RT_CHUNK ? rt_lane(sethi, l + 1) : nhi;
                    if (lane == nrows) { A = delta; B = 1.0; C = -hi1; }
                    const double w = rt_wave_min(A > 0.0 ? rt_w_max(A, B, C, x) : INFINITY);
                    const double x1 = fmin(fmax(x + delta * w, lo1), hi1);
                    t += rt_dt(T, delta, x, x1);
                    x = x1;
                } else {
                    if (lane == 0 && legT) legT[ls] = t;
                    Ttot = leg == 0 ? t : Ttot + t;
                }
                continue;
            }
            double cap = rec[RT_CAP * RT_STRIDE + l];
            if (narm == 2) cap = fmin(cap, rec[(RT_NF + RT_CAP) * RT_STRIDE + l]);
            int moving = 0;
            if ((kk == 0 && leg == 0) || (kk == n && leg == M))
                moving = __any(lane < nq && rec[((lane / 7) * RT_NF + RT_V + lane % 7) * RT_STRIDE + l] != 0.0);
            RtSet S = {0.0, INFINITY, 0};
            if (kk < n) {
                if (lane == nrows) { A = delta; B = 1.0; C = -hi1; }
                if (lane == nrows + 1) { A = -delta; B = -1.0; C = lo1; }
            }
            if (A == 0.0) rt_cut_x(S, B, C);
            if (kk < n) {
                for (int jj = 0; jj < nrows + 2; jj++) {
                    const double Aj = rt_lane(A, jj);
                    if (!(Aj < 0.0)) continue;
                    const double Bj = rt_lane(B, jj), Cj = rt_lane(C, jj);
                    if (A > 0.0) rt_cut_pair(S, A, B, C, Aj, Bj, Cj);
                }
            }
            double lo = rt_wave_max(S.lo), hi = fmin(rt_wave_min(S.hi), cap);
            if (kk == n && leg < M) { lo = fmax(lo, lo1); hi = fmin(hi, hi1); }        // a junction: within K_0 of the later leg
            bool fail = __any(S.empty) || !(lo <= hi) || hi == 0.0;
            if (moving) {                           // a pinned end of the route
                fail = fail || !(lo <= 1.0 && 1.0 <= hi);
                if (kk == n) lo = hi = 1.0;
                else pin0 = 1;
            }
            if (fail) { status = MPCMP_RT_INFEASIBLE; leg_fail = leg; k_fail = kk; break; }
            lo1 = lo; hi1 = hi;
            if (lane == l) { mine0 = lo; mine1 = hi; }
        }
        if (!status && lane < npt) { pf[2 * k] = mine0; pf[2 * k + 1] = mine1; }
        __syncthreads();
    }
    if (!status && !rt_finite(Ttot)) status = MPCMP_RT_INFEASIBLE;
    if (status) {
        for (int m = 0; m < nl; m++) {
            double *pf = prof + (l0 + m) * (n + 1) * 2;
            for (int k = lane; k <= n; k += RT_NT) { pf[2 * k] = qnan; pf[2 * k + 1] = qnan; }
            if (lane == 0 && legT) legT[l0 + m] = INFINITY;
        }
    }
    if (lane == 0) {
        mpcmp_route_retime r = rrt_failed(status, leg_fail, k_fail);
        if (!status) { r.T_new = Ttot; r.rate_min = sqrt(xmin); r.s_slowest = (double)kmin / n; r.leg_slowest = legmin; r.n_slowed = nslow; }
        if (rout) rout[b] = r;
        else pout[b] = rt_plan_record(r);
    }
}

// One thread per (route, sample): the retimed leg durations are the last t of every leg's profile; the leg of the route time by a sequential
// prefix sum over them, then the interval of the leg time by bisection on the t_k of that leg's profile and the retimed-sample rule.
__global__ __launch_bounds__(128) void k_sample_retimed(const mpcmp_model *__restrict__ mdl, int mstride, int narm, int nseg, int B, int M, int n,
                                                        int n_pts, const double *__restrict__ sx, const double *__restrict__ su,
                                                        const double *__restrict__ sT, const double *__restrict__ prof, double *__restrict__ out) {
    const long idx = (long)blockIdx.x * 128 + threadIdx.x;
    if (idx >= (long)B * (n_pts + 1)) return;
    const int b = (int)(idx / (n_pts + 1)), i = (int)(idx % (n_pts + 1)), N = 3 * nseg + 1, nq = 7 * narm, W = 1 + 28 * narm, nl = M + 1;
    const size_t l0 = (size_t)b * nl, ps = (size_t)(n + 1) * 2;
    double *o = out + (size_t)idx * W;
    double Tn = 0.0;
    bool finite = true;
    for (int m = 0; m < nl; m++) { const double D = prof[(l0 + m) * ps + 2 * n]; Tn = m ? Tn + D : D; finite = finite && rt_finite(D); }
    if (!finite) {
        for (int e = 0; e < W; e++) o[e] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const double t = ((double)i / n_pts) * Tn;
    double Ep = 0.0;
    int leg = 0;
    for (;;) {
        const double E = Ep + prof[(l0 + leg) * ps + 2 * n];
        if (t < E || leg == nl - 1) break;
        Ep = E; leg++;
    }
    if (i == n_pts) leg = M;
    const size_t ls = l0 + leg;
    const double *pf = prof + ls * ps;
    const double T = sT[ls], tl = fmin(fmax(t - Ep, 0.0), pf[2 * n]);
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pf[2 * mid] <= tl) lo = mid; else hi = mid - 1;
    }
    int k = lo;
    if (i == n_pts) k = n - 1;
    const double tk = pf[2 * k], xk = pf[2 * k + 1], x1 = pf[2 * k + 3], lk = sqrt(xk), w = (x1 - xk) * n, h = 0.5 / T;
    double lam = lk + w * (tl - tk) * h, s = (double)k / n + (tl - tk) * (lk + lam) * h;
    if (i == n_pts) { lam = sqrt(x1); s = 1.0; }
    s = fmin(fmax(s, 0.0), 1.0);
    const double xs = lam * lam;
    const double *X = sx + ls * N * 2 * nq, *U = su + ls * N * nq;
    double Lg[4];
    const int seg = lagrange_segment(nseg, s, Lg);
    o[0] = t;
    for (int a = 0; a < narm; a++) {
        double q[7], v[7], ac[7], sc[14], qd[7], qdd[7], tau[7];
        interp_joints(X + 7 * a, X + nq + 7 * a, 2 * nq, U + 7 * a, nq, seg, Lg, q, v, ac, sc);
#pragma unroll
        for (int r = 0; r < 7; r++) { qd[r] = lam * v[r]; qdd[r] = xs * ac[r] + w * h * v[r]; }
        rnea_dir<false>(mdl + ls * mstride + a, sc, qd, qdd, 0, 0, tau, nullptr);
#pragma unroll
        for (int r = 0; r < 7; r++) { o[1 + 28 * a + r] = q[r]; o[8 + 28 * a + r] = qd[r]; o[15 + 28 * a + r] = qdd[r]; o[22 + 28 * a + r] = tau[r]; }
    }
}

static bool rt_shape_ok(int narm, int nseg, int B, int M, int n_grid) {
    return narm >= 1 && narm <= RT_MAX_ARMS && nseg >= 1 && 3 * nseg + 1 <= RT_MAX_NODES && n_grid >= 1 && n_grid <= RT_MAX_GRID && B >= 1 && M >= 0;
}

hipError_t retime_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, const mpcmp_bounds *rows,
                         const mpcmp_bounds &table, const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_retime_spec &spec,
                         double *d_prof, double *d_leg_T, mpcmp_retime *d_plan_out, mpcmp_route_retime *d_route_out, hipStream_t st) {
    if (!rt_shape_ok(narm, nseg, B, M, n_grid) || !d_plan_out == !d_route_out || (d_plan_out && M)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_retime, dim3(B), dim3(RT_NT), 0, st, mdl, mstride, narm, nseg, n_grid, M, rows, table, d_sx, d_su, d_sT, spec, d_prof,
                       d_leg_T, d_plan_out, d_route_out);
    return hipGetLastError();
}

hipError_t sample_retimed_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int M, int n_grid, int n_pts, const double *d_sx,
                                 const double *d_su, const double *d_sT, const double *d_prof, double *d_out, hipStream_t st) {
    if (!rt_shape_ok(narm, nseg, B, M, n_grid) || n_pts < 1) return hipErrorInvalidValue;
    const long total = (long)B * (n_pts + 1);
    hipLaunchKernelGGL(k_sample_retimed, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, st, mdl, mstride, narm, nseg, B, M, n_grid, n_pts, d_sx,
                       d_su, d_sT, d_prof, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host statement (no GPU): the records from plain host C++, then the row, pair and clock arithmetic of retime.hpp ----
// The rule over n_legs legs: rows [n_legs], x, u and prof leg after leg, T [n_legs]; leg_T_new may be NULL.
static int retime_legs_host(const mpcmp_model *models, int narm, int num_seg, int n_legs, const mpcmp_bounds *rows, const mpcmp_retime_spec *spec,
                            const double *x, const double *u, const double *T, int n_grid, double *prof, double *leg_T_new, mpcmp_route_retime *out) {
    if (!models || narm < 1 || narm > RT_MAX_ARMS || num_seg < 1 || 3 * num_seg + 1 > RT_MAX_NODES || n_legs < 1 || !rows || !x || !u || !T ||
        n_grid < 1 || n_grid > RT_MAX_GRID || !prof || !out) return MPCMP_EINVAL;
    const mpcmp_retime_spec sp = spec ? *spec : rt_default_spec();
    if (!rt_spec_ok(sp)) return MPCMP_EINVAL;
    const int n = n_grid, N = 3 * num_seg + 1, nq = 7 * narm, nrows = RT_ROWS_ARM * narm, nl = n_legs, Mlast = n_legs - 1;
    const size_t P = (size_t)n + 1;                      // points per leg
    auto fail_with = [&](int status, int leg, int k) {
        for (size_t e = 0; e < 2 * P * nl; e++) prof[e] = NAN;
        if (leg_T_new) for (int m = 0; m < nl; m++) leg_T_new[m] = INFINITY;
        *out = rrt_failed(status, leg, k);
        return MPCMP_OK;
    };
    bool bad = false;
    for (int m = 0; m < nl; m++) bad = bad || !(std::isfinite(T[m]) && T[m] > 0.0);
    for (size_t e = 0; e < (size_t)nl * 2 * nq * N; e++) bad = bad || !std::isfinite(x[e]);
    for (size_t e = 0; e < (size_t)nl * nq * N; e++) bad = bad || !std::isfinite(u[e]);
    if (bad) return fail_with(MPCMP_RT_NAN, -1, -1);

    std::vector<double> rec(P * nl * narm * RT_NF), Klo(P * nl), Khi(P * nl);
    for (int m = 0; m < nl; m++) {
        const double *xm = x + (size_t)m * N * 2 * nq, *um = u + (size_t)m * N * nq, *bd = reinterpret_cast<const double *>(rows + m);
        for (int k = 0; k <= n; k++) {
            double Lg[4];
            const int s = mpcmp_plan::lagrange_segment(num_seg, (double)k / n, Lg);
            for (int a = 0; a < narm; a++) {
                double q[7], v[7], ac[7], tc[7], t1[7], t2[7], J[42], p[3], R[9], tw[6];
                const double zero[7] = {0, 0, 0, 0, 0, 0, 0};
                mpcmp_plan::interp_qva(xm + 7 * a, xm + nq + 7 * a, 2 * nq, um + 7 * a, nq, s, Lg, q, v, ac);
                mpcmp_host::rnea_host(models[a], q, zero, zero, tc);
                mpcmp_host::rnea_host(models[a], q, v, ac, t1);
                mpcmp_host::rnea_host(models[a], q, zero, v, t2);
                mpcmp_host::tool_jacobian(models[a], q, J, p, R);
                for (int r = 0; r < 6; r++) { tw[r] = 0.0; for (int j = 0; j < 7; j++) tw[r] += J[7 * r + j] * v[j]; }
                rt_record(bd, sp, v, ac, tc, t1, t2, std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]),
                          std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]), &rec[((m * P + k) * narm + a) * RT_NF], 1);
            }
        }
    }
    const double delta = 1.0 / n, rmax2 = sp.rate_max * sp.rate_max;
    double A[RT_ROWS_ARM * RT_MAX_ARMS + 2], Bc[RT_ROWS_ARM * RT_MAX_ARMS + 2], Cc[RT_ROWS_ARM * RT_MAX_ARMS + 2];
    auto point_rows = [&](int m, int k) {
        const double *bd = reinterpret_cast<const double *>(rows + m);
        const double h = 0.5 / T[m];
        for (int r = 0; r < nrows; r++) rt_row(&rec[((m * P + k) * narm + r / RT_ROWS_ARM) * RT_NF], 1, bd, h, sp.groups, r % RT_ROWS_ARM, A[r], Bc[r], Cc[r]);
    };
    auto moving = [&](int m, int k) { for (int a = 0; a < narm; a++) for (int j = 0; j < 7; j++) if (rec[((m * P + k) * narm + a) * RT_NF + RT_V + j] != 0.0) return true; return false; };
    auto cap_of = [&](int m, int k) { double c = INFINITY; for (int a = 0; a < narm; a++) c = fmin(c, rec[((m * P + k) * narm + a) * RT_NF + RT_CAP]); return c; };
    const bool pin0 = moving(0, 0), pinn = moving(Mlast, n);
    // backward
    for (int m = Mlast; m >= 0; m--) {
        for (int k = n; k >= 0; k--) {
            point_rows(m, k);
            int nr = nrows;
            if (k < n) { A[nr] = delta; Bc[nr] = 1.0; Cc[nr] = -Khi[m * P + k + 1]; nr++; A[nr] = -delta; Bc[nr] = -1.0; Cc[nr] = Klo[m * P + k + 1]; nr++; }
            RtSet S = {0.0, INFINITY, 0};
            for (int i = 0; i < nr; i++) {
                if (A[i] == 0.0) rt_cut_x(S, Bc[i], Cc[i]);
                if (k < n && A[i] > 0.0) for (int j = 0; j < nr; j++) if (A[j] < 0.0) rt_cut_pair(S, A[i], Bc[i], Cc[i], A[j], Bc[j], Cc[j]);
            }
            double lo = S.lo, hi = fmin(S.hi, cap_of(m, k));
            if (k == n && m < Mlast) { lo = fmax(lo, Klo[(m + 1) * P]); hi = fmin(hi, Khi[(m + 1) * P]); }
            bool fail = S.empty || !(lo <= hi) || hi == 0.0;
            if ((k == n && m == Mlast && pinn) || (k == 0 && m == 0 && pin0)) {
                fail = fail || !(lo <= 1.0 && 1.0 <= hi);
                if (k == n) lo = hi = 1.0;
            }
            if (fail) return fail_with(MPCMP_RT_INFEASIBLE, m, k);
            Klo[m * P + k] = lo; Khi[m * P + k] = hi;
        }
    }
    // forward
    double xk = pin0 ? 1.0 : Khi[0], Ttot = 0.0, xmin = INFINITY;
    int kmin = 0, legmin = 0, nslow = 0;
    for (int m = 0; m < nl; m++) {
        double t = 0.0;
        double *pf = prof + 2 * P * m;
        for (int k = 0; k <= n; k++) {
            if (xk < xmin) { xmin = xk; kmin = k; legmin = m; }
            if ((k > 0 || m == 0) && xk < rmax2) nslow++;
            pf[2 * k] = t; pf[2 * k + 1] = xk;
            if (k == n) break;
            point_rows(m, k);
            double w = rt_w_max(delta, 1.0, -Khi[m * P + k + 1], xk);
            for (int r = 0; r < nrows; r++) if (A[r] > 0.0) w = fmin(w, rt_w_max(A[r], Bc[r], Cc[r], xk));
            const double x1 = fmin(fmax(xk + delta * w, Klo[m * P + k + 1]), Khi[m * P + k + 1]);
            t += rt_dt(T[m], delta, xk, x1);
            xk = x1;
        }
        if (leg_T_new) leg_T_new[m] = t;
        Ttot = m == 0 ? t : Ttot + t;
    }
    if (!std::isfinite(Ttot)) return fail_with(MPCMP_RT_INFEASIBLE, -1, -1);
    mpcmp_route_retime r = rrt_failed(0, -1, -1);
    r.T_new = Ttot; r.rate_min = std::sqrt(xmin); r.s_slowest = (double)kmin / n; r.leg_slowest = legmin; r.n_slowed = nslow;
    *out = r;
    return MPCMP_OK;
}

extern "C" int mpcmp_retime_route_one(const mpcmp_model *models, int narm, int num_seg, int n_legs, const mpcmp_bounds *rows,
                                      const mpcmp_retime_spec *spec, const double *x, const double *u, const double *T, int n_grid, double *prof,
                                      double *leg_T_new, mpcmp_route_retime *out) {
    return retime_legs_host(models, narm, num_seg, n_legs, rows, spec, x, u, T, n_grid, prof, leg_T_new, out);
}

// a plan is a route of one leg with one bounds row; its record is that route's without the leg fields
extern "C" int mpcmp_retime_one(const mpcmp_model *models, int narm, int num_seg, const mpcmp_bounds *row, const mpcmp_retime_spec *spec,
                                const double *x, const double *u, double T, int n_grid, double *prof, mpcmp_retime *out) {
    if (!out) return MPCMP_EINVAL;
    mpcmp_route_retime r;
    if (int rc = retime_legs_host(models, narm, num_seg, 1, row, spec, x, u, &T, n_grid, prof, nullptr, &r)) return rc;
    *out = rt_plan_record(r);
    return MPCMP_OK;
}
