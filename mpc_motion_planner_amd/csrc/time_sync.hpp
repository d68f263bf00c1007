// time_sync.hpp — kernels of the time scaling of trajectories and of the time-synchronised solve (mpcmp_time_scale_batch*,
// mpcmp_solve_batch_synced*; include/mpcmp.h).  All of them write with plain stores.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "solver_types.hpp"

namespace mpcmp {

// Stretch B trajectories [N][14 narm] / [N][7 narm] / T to T_new (collocation is in normalised time: the nodes keep their positions), then pin node 0
// to x0 and node N - 1 to xf (motionPlanner.cpp:199-207).  Per problem, s = T / T_new (one IEEE division); interior nodes: q unchanged, qd * s;
// every node's u * (s * s); oT = T_new.  One workgroup per problem: every thread forms s before the barrier, and oT is written after it, so the
// outputs may be the inputs (oT == sT included).  skip (or null): problems with skip[b] != 0 are not written.
__global__ __launch_bounds__(256) void k_time_scale(int N, int narm, const double *x0, const double *xf, const double *sx, const double *su,
                                                    const double *sT, const double *T_new, const int *skip, double *ox, double *ou, double *oT) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (skip != nullptr && skip[b] != 0) return;          // (uniform: the whole workgroup leaves)
    const int nx = 14 * narm, nu = 7 * narm;
    const double T1 = T_new[b], s = sT[b] / T1;
    for (int e = tid; e < nx * N; e += blockDim.x) {
        const int k = e / nx, c = e % nx;
        double v;
        if (k == 0) v = x0[(size_t)b * nx + c];
        else if (k == N - 1) v = xf[(size_t)b * nx + c];
        else {
            v = sx[(size_t)b * nx * N + e];
            if (c >= 7 * narm) v = v * s;          // (columns [7 narm, 14 narm): the joint velocities of every arm)
        }
        ox[(size_t)b * nx * N + e] = v;
    }
    for (int q = tid; q < nu * N; q += blockDim.x) ou[(size_t)b * nu * N + q] = su[(size_t)b * nu * N + q] * (s * s);
    __syncthreads();                                     // (every thread has read sT[b])
    if (tid == 0) oT[b] = T1;
}

// A double as an unsigned key with the same order (negative values: all bits flipped; the others: the sign bit set).  Key 0 lies below every
// double, so zeroed slots are empty; an atomicMax over keys is independent of the order of its arrivals, hence deterministic.
__device__ __forceinline__ unsigned long long t_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double t_of_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
// a problem takes part in its group's common time: a group id in [0, n_groups) and a pass-1 solve without a hard failure (MPCMP_ST_FAILED)
__device__ __forceinline__ bool sync_eligible(int g, int n_groups, int status) {
    return g >= 0 && g < n_groups && (status & MPCMP_ST_FAILED) == 0;
}

// segmented maximum of the pass-1 final times over the eligible members of each group; gkey / gcount [n_groups] zeroed on the stream before
__global__ __launch_bounds__(256) void k_sync_tmax(int B, const int *group, int n_groups, const int *status, const double *sT,
                                                   unsigned long long *gkey, int *gcount) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int g = group[i];
    if (!sync_eligible(g, n_groups, status[i])) return;
    atomicMax(gkey + g, t_key(sT[i]));
    atomicAdd(gcount + g, 1);
}

// After k_sync_tmax: group_T [n_groups] (NaN for a group without an eligible member; group_T may be null), and per problem the pass-2 mask skip
// (0 = re-solved: eligible with a pass-1 T below its group's), the pass-2 window rows [B][2] = (group_T, group_T) and T_new [B] = group_T of the
// re-solved.  A skipped problem's row and T_new hold its pass-1 T (finite values, read by no kernel whose results are kept).
// The pass-1 status words are kept (saved [B]) and put back for the skipped problems after pass 2 (k_sync_restore): at N = 25 their QP kernels still
// run in pass 2 and add to the word, which the next solve reads (prev_bad: carried multipliers, re-guess)
__global__ __launch_bounds__(256) void k_sync_prepare(int B, const int *group, int n_groups, const int *status, const double *sT,
                                                      const unsigned long long *gkey, const int *gcount, double *group_T, int *skip,
                                                      double *rows, double *T_new, int *saved) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (group_T != nullptr && i < n_groups) group_T[i] = gcount[i] > 0 ? t_of_key(gkey[i]) : __longlong_as_double(0x7FF8000000000000ll);
    if (i >= B) return;
    const int g = group[i];
    const double T = sT[i];
    double Tg = T;
    int re = 0;
    if (sync_eligible(g, n_groups, status[i])) {
        const double m = t_of_key(gkey[g]);
        if (T < m) { Tg = m; re = 1; }
    }
    skip[i] = !re;
    rows[2 * i] = Tg; rows[2 * i + 1] = Tg;
    T_new[i] = Tg;
    saved[i] = status[i];
}

// after pass 2: the skipped problems' status words as pass 1 left them
__global__ __launch_bounds__(256) void k_sync_restore(int B, const int *skip, const int *saved, int *status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B && skip[i] != 0) status[i] = saved[i];
}

}  // namespace mpcmp
