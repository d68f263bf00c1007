// limits.hpp — what the between-node limit checker shares between the host entry points (mpcmp.hip), its kernel (limits.hip) and the host
// restatement mpcmp_limits_config: the excess and ratio formulas, the ordering of ties, the per-thread accumulator and the launcher.
// The kernel itself lives in limits.hip, a translation unit of its own: nothing here is a kernel, so including this header does not change what
// any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/mpcmp.h"

namespace mpcmp {

constexpr int LIM_MAX_PTS = 4096;    // n_pts
constexpr int LIM_NT = 256;          // threads per workgroup of k_limits
constexpr int LIM_MAX_NODES = 25;    // 3 num_seg + 1 for num_seg <= 8
constexpr int LIM_MAX_ARMS = 2;

// neither NaN nor infinite (one text for host and device)
__host__ __device__ inline bool lim_finite(double x) { return x - x == 0.0; }

// excess of x over [lb, ub]: negative = inside by that much; -inf when both bounds are infinite
__host__ __device__ inline double lim_excess(double x, double lb, double ub) { return fmax(x - ub, lb - x); }

// the factor by which x has to shrink to meet the bound on its side: 0 when that bound is infinite, +inf when no slowing down meets it
__host__ __device__ inline double lim_ratio(double x, double lb, double ub) {
    if (x > 0.0) return ub == INFINITY ? 0.0 : (ub <= 0.0 ? INFINITY : x / ub);
    if (x < 0.0) return lb == -INFINITY ? 0.0 : (lb >= 0.0 ? INFINITY : x / lb);
    return 0.0;
}
// the same for a speed v >= 0 against a maximum >= 0
__host__ __device__ inline double lim_tool_ratio(double v, double mx) { return (mx == INFINITY || !(v > 0.0)) ? 0.0 : (mx <= 0.0 ? INFINITY : v / mx); }

// Ties of an excess: lowest sample, then lowest channel = the order of this key.  sample < 2^13, channel < 2^4.
__host__ __device__ inline unsigned lim_pack(int ip, int channel) { return ((unsigned)ip << 4) | (unsigned)channel; }
constexpr unsigned LIM_NO_KEY = 0xFFFFFFFFu;
__host__ __device__ inline bool lim_better(double e, unsigned k, double be, unsigned bk) { return e > be || (e == be && k < bk); }

// What a thread keeps over its samples (and mpcmp_limits_config over its one): per group the best (excess, key) pair, the four stretch ratios
// r_v, r_a, r_lin, r_ang, the count and first index of violating samples, and whether a value was not finite.
struct LimAcc {
    double ex[MPCMP_LIM_GROUPS];
    unsigned key[MPCMP_LIM_GROUPS];
    double r[4];
    int n_viol, first, nan;
};
constexpr int LIM_NO_SAMPLE = 0x7FFFFFFF;
__host__ __device__ inline void lim_init(LimAcc &A) {
    for (int g = 0; g < MPCMP_LIM_GROUPS; g++) { A.ex[g] = -INFINITY; A.key[g] = LIM_NO_KEY; }
    for (int k = 0; k < 4; k++) A.r[k] = 0.0;
    A.n_viol = 0; A.first = LIM_NO_SAMPLE; A.nan = 0;
}
// one channel of group g; returns whether it is over the group's tolerance.  An excess of -inf (no bound) never takes the key.
__host__ __device__ inline bool lim_fold(LimAcc &A, int g, double e, unsigned k, double tol) {
    if (e > -INFINITY && lim_better(e, k, A.ex[g], A.key[g])) { A.ex[g] = e; A.key[g] = k; }
    return e > tol;
}

// The values of one arm at sample ip folded into A: q, qd, qdd, tau [7], the tool height z and the tool speeds vlin, vang >= 0, under the bounds row
// `bd` [58] (the layout of mpcmp_bounds: lbx 14, ubx 14, lbu 7, ubu 7, lbg 8, ubg 8).  Returns whether some group of this arm is over its tolerance.
__host__ __device__ inline bool lim_fold_arm(LimAcc &A, const double *bd, const mpcmp_limits_spec &sp, int ip, int arm, const double *q,
                                             const double *qd, const double *qdd, const double *tau, double z, double vlin, double vang) {
    const double *lbx = bd, *ubx = bd + 14, *lbu = bd + 28, *ubu = bd + 35, *lbg = bd + 42, *ubg = bd + 50;
    bool over = false, bad = !lim_finite(z) || !lim_finite(vlin) || !lim_finite(vang);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 7; j++) {
        const unsigned k = lim_pack(ip, 7 * arm + j);
        bad = bad || !lim_finite(q[j]) || !lim_finite(qd[j]) || !lim_finite(qdd[j]) || !lim_finite(tau[j]);
        over |= lim_fold(A, MPCMP_LIM_Q, lim_excess(q[j], lbx[j], ubx[j]), k, sp.tol[MPCMP_LIM_Q]);
        over |= lim_fold(A, MPCMP_LIM_QD, lim_excess(qd[j], lbx[7 + j], ubx[7 + j]), k, sp.tol[MPCMP_LIM_QD]);
        over |= lim_fold(A, MPCMP_LIM_QDD, lim_excess(qdd[j], lbu[j], ubu[j]), k, sp.tol[MPCMP_LIM_QDD]);
        over |= lim_fold(A, MPCMP_LIM_TAU, lim_excess(tau[j], lbg[j], ubg[j]), k, sp.tol[MPCMP_LIM_TAU]);
        A.r[0] = fmax(A.r[0], lim_ratio(qd[j], lbx[7 + j], ubx[7 + j]));
        A.r[1] = fmax(A.r[1], lim_ratio(qdd[j], lbu[j], ubu[j]));
    }
    const unsigned ka = lim_pack(ip, arm);
    over |= lim_fold(A, MPCMP_LIM_HEIGHT, lim_excess(z, lbg[7], ubg[7]), ka, sp.tol[MPCMP_LIM_HEIGHT]);
    over |= lim_fold(A, MPCMP_LIM_TOOL_LIN, vlin - sp.tool_lin_max, ka, sp.tol[MPCMP_LIM_TOOL_LIN]);
    over |= lim_fold(A, MPCMP_LIM_TOOL_ANG, vang - sp.tool_ang_max, ka, sp.tol[MPCMP_LIM_TOOL_ANG]);
    A.r[2] = fmax(A.r[2], lim_tool_ratio(vlin, sp.tool_lin_max));
    A.r[3] = fmax(A.r[3], lim_tool_ratio(vang, sp.tool_ang_max));
    if (bad) A.nan = 1;
    return over;
}
// a sample (all its arms folded) that is over some tolerance
__host__ __device__ inline void lim_count(LimAcc &A, int ip, bool over) {
    if (over) { A.n_viol++; if (ip < A.first) A.first = ip; }
}
__host__ __device__ inline double lim_stretch(const double *r) { return fmax(fmax(1.0, r[0]), fmax(sqrt(r[1]), fmax(r[2], r[3]))); }

// the spec a NULL pointer stands for
inline mpcmp_limits_spec lim_default_spec() {
    mpcmp_limits_spec s;
    for (int g = 0; g < MPCMP_LIM_GROUPS; g++) s.tol[g] = 0.0;
    s.tool_lin_max = s.tool_ang_max = INFINITY;
    return s;
}
// finite tolerances, tool maxima neither NaN nor negative
inline bool lim_spec_ok(const mpcmp_limits_spec &s) {
    for (int g = 0; g < MPCMP_LIM_GROUPS; g++) if (!std::isfinite(s.tol[g])) return false;
    return s.tool_lin_max >= 0.0 && s.tool_ang_max >= 0.0;
}

// mdl / mstride as k_sample takes them (problem b, arm a: mdl + b * mstride + a); rows [B] or NULL: then `table`, the configuration's, for everyone
hipError_t limits_launch(const mpcmp_model *mdl, int mstride, int narm, int nseg, int B, int n_pts, const mpcmp_bounds *rows, const mpcmp_bounds &table,
                         const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_limits_spec &spec, mpcmp_limits *d_out, hipStream_t st);

}  // namespace mpcmp
