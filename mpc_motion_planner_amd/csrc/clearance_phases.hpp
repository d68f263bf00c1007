// clearance_phases.hpp — the phases the sampled clearance kernels share (k_clearance of clearance.hip, the three kernels of moving.hip,
// k_clearance_field of field.hip), on the layout of clearance_lds.hpp: staging, A1 + A2 of a chunk, the pair phase, the hit count and the
// workgroup reduction (which the certified kernel uses as well).  Device functions only, inlined into their kernels: nothing here is a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "clearance.hpp"
#include "clearance_cert.hpp"
#include "plan_interp.hpp"

namespace mpcmp {

inline ClrShape clr_shape(const ClrTables &t, bool with_obs) {
    ClrShape h;
    h.narm = t.narm; h.nseg = t.nseg; h.n0 = t.n_sph[0]; h.n1 = t.n_sph[1];
    h.n_obs = with_obs ? t.n_obs : 0; h.obs_stride = with_obs ? t.obs_stride : 0;
    h.chunk = clr_chunk(h.n0 + h.n1);
    return h;
}

// the tables of problem b into LDS: joint placements, position nodes, spheres, obstacles, the hit flags cleared.  Returns whether this thread saw a
// position node that is not finite (the kernels that flag a NaN by the interpolated sample do not ask).  The caller's barrier follows
__device__ __forceinline__ bool clr_stage(const ClrLds &L, const ClrShape &h, const mpcmp_model *__restrict__ mdl, const ClrSphere *__restrict__ sph,
                                          const mpcmp_obstacle *__restrict__ obs, const double *__restrict__ sx, int b) {
    const int tid = threadIdx.x, N = 3 * h.nseg + 1, nq = 7 * h.narm, nsph = h.n0 + h.n1;
    for (int e = tid; e < 84 * h.narm; e += CLR_NT) {
        const int a = e / 84, i = (e % 84) / 12, c = e % 12;
        L.mk[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    const double *X = sx + (size_t)b * N * 2 * nq;
    bool bad = false;
    for (int e = tid; e < nq * N; e += CLR_NT) {
        const double v = X[(size_t)(e / nq) * 2 * nq + e % nq];
        L.nodes[e] = v;
        bad = bad || !isfinite(v);
    }
    for (int s = tid; s < nsph; s += CLR_NT) {
        const ClrSphere S = sph[s];
        L.sk[4 * s] = S.c[0]; L.sk[4 * s + 1] = S.c[1]; L.sk[4 * s + 2] = S.c[2]; L.sk[4 * s + 3] = S.r;
        L.sj[s] = 7 * S.arm + S.joint;
        if (L.sa) L.sa[s] = S.arm;
    }
    const mpcmp_obstacle *O = obs + (size_t)b * h.obs_stride;
    for (int o = tid; o < h.n_obs; o += CLR_NT) {
        clr_obs_prepare(O[o], L.ok + 8 * o);
        L.ot[o] = O[o].type;
    }
    for (int e = tid; e < h.chunk; e += CLR_NT) L.hit[e] = 0;
    return bad;
}

// phases A1 and A2 of a chunk of ns samples, sample sl at the normalised time time_of(sl): one thread per (sample, joint) for the node interpolant
// of the joint position and its sine / cosine, then one per (sample, arm) for the chain of frames.  nan_flag (LDS, or null) is set by an
// interpolated position that is not finite.  Ends with a barrier
template <class TimeOf>
__device__ __forceinline__ void clr_frames(const ClrLds &L, const ClrShape &h, int ns, TimeOf time_of, int *nan_flag) {
    const int tid = threadIdx.x, nq = 7 * h.narm;
    for (int it = tid; it < ns * nq; it += CLR_NT) {
        const int sl = it / nq, j = it % nq;
        double Lg[4];
        const int s = mpcmp_plan::lagrange_segment(h.nseg, time_of(sl), Lg);
        const double q = mpcmp_plan::interp_channel(L.nodes + j, nq, s, Lg);
        if (nan_flag && !isfinite(q)) *nan_flag = 1;
        double sn, cs;
        sincos(q, &sn, &cs);
        L.sc[2 * it] = sn; L.sc[2 * it + 1] = cs;
    }
    __syncthreads();
    for (int it = tid; it < ns * h.narm; it += CLR_NT) {
        const int sl = it / h.narm, a = it % h.narm;
        cert_frames(L.mk + 84 * a, L.sc + (size_t)(sl * nq + 7 * a) * 2, L.fr + (size_t)(sl * nq + 7 * a) * 12);
    }
    __syncthreads();
}

// the world centre c [3] of (sample sl, sphere s) from the chunk's frames
__device__ __forceinline__ void clr_centre(const ClrLds &L, const ClrShape &h, int sl, int s, double *c) {
    cert_centre(L.fr + (size_t)(sl * 7 * h.narm + L.sj[s]) * 12, L.sk + 4 * s, c);
}

// phase C of a chunk: the smallest robot-pair clearance of (sample sl, sphere s) and its partner
__device__ __forceinline__ double clr_pairs(const ClrLds &L, int nsph, int sl, int s, int self_gap, int *tm) {
    const double *C = L.cen + (size_t)sl * nsph * 3;
    const double cx = C[3 * s], cy = C[3 * s + 1], cz = C[3 * s + 2], rs = L.sk[4 * s + 3];
    const int as = L.sa[s], js = L.sj[s];
    double dm = INFINITY;
    *tm = 0;
    for (int t = s + 1; t < nsph; t++) {
        if (!clr_pair(as, js, L.sa[t], L.sj[t], self_gap)) continue;      // (sj holds arm * 7 + joint: differences within one arm are joint differences)
        const double ex = cx - C[3 * t], ey = cy - C[3 * t + 1], ez = cz - C[3 * t + 2];
        const double d = sqrt(ex * ex + ey * ey + ez * ez) - rs - L.sk[4 * t + 3];
        if (d < dm) { dm = d; *tm = t; }
    }
    return dm;
}

// one thread, after the chunk's last barrier: the hit flags of the ns samples from ip0 on into the count and the first hit, cleared for the next chunk
__device__ __forceinline__ void clr_count_hits(const ClrLds &L, int ns, int ip0, int *first, int *n_hit) {
    for (int sl = 0; sl < ns; sl++) {
        if (L.hit[sl]) { if (*first < 0) *first = ip0 + sl; ++*n_hit; }
        L.hit[sl] = 0;
    }
}

// Workgroup reduction of every thread's best (clearance, key) by clr_better; thread 0 holds the result.  pay (or null): an int carried beside the
// key (the voxel of k_clearance_field).  The keys order the result, so it does not depend on the launch or on the batch
template <class K> __device__ __forceinline__ void clr_reduce(double &best_d, K &best_k, int *pay) {
    __shared__ double red_d[CLR_NT / 64];
    __shared__ K red_k[CLR_NT / 64];
    __shared__ int red_v[CLR_NT / 64];
    const int tid = threadIdx.x;
    int v = pay ? *pay : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(best_d, off);
        const K ok = __shfl_down(best_k, off);
        const int ov = pay ? __shfl_down(v, off) : 0;
        if (clr_better(od, ok, best_d, best_k)) { best_d = od; best_k = ok; v = ov; }
    }
    if ((tid & 63) == 0) { red_d[tid >> 6] = best_d; red_k[tid >> 6] = best_k; if (pay) red_v[tid >> 6] = v; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CLR_NT / 64; w++)
            if (clr_better(red_d[w], red_k[w], best_d, best_k)) { best_d = red_d[w]; best_k = red_k[w]; if (pay) v = red_v[w]; }
        if (pay) *pay = v;
    }
}

}  // namespace mpcmp
