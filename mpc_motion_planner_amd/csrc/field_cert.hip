// field_cert.hip — the kernels of the certified clearance check against a voxel world (include/mpcmp_field_cert.h): k_clearance_cert_field and the
// certificate merge k_clearance_cert_merge.  The rule is field_cert_rule.hpp on top of clearance_cert.hpp and field_rule.hpp, which the host
// statement in model_host.cpp runs as well.  A translation unit of its own, so that every other unit compiles exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "field_cert.hpp"
#include "clearance_phases.hpp"

namespace mpcmp {

// One workgroup per plan, the structure of cert_search (clearance_cert.hip).  Staged in LDS once: the joint placements, the position nodes, the
// sphere tables with their reach.  Two lists of interval indices in LDS, the current level's and the next one's, both in time order.  A level runs
// in chunks of `chunk` intervals, four phases per chunk:
//   A1  one thread per (interval, joint): q(t_m) with its sine / cosine, and dev (cert_deviation);
//   A2  one thread per (interval, arm): the frames of the arm at t_m (cert_frames), once per interval;
//   B   one thread per (interval, sphere): the world centre, ONE entry of the field from global memory (its address depends on the centre, so the
//       load is issued before D_s is summed from LDS), d_s and d_s - D_s into the sphere's row of the chunk;
//   D   one lane of the first wave per interval: the minima over the spheres, the decision, and the children of the intervals to be split appended
//       to the next list at the rank a ballot gives them: time order and the capacity rule without a counter that threads race for.
// There is no phase C: the field check knows no robot pairs.  Every thread keeps its best (d, key, voxel) in registers over all chunks and levels,
// the deciding lanes their leaf counts and best (L, key); one reduction at the end, ordered by the keys, so the records do not depend on the launch
// or on the batch.  No atomics.  sol_T is read for the time fields only.
__global__ __launch_bounds__(CLR_NT) void k_clearance_cert_field(const mpcmp_model *__restrict__ mdl, FcertShape h, const ClrSphere *__restrict__ sph,
                                                                 mpcmp_field_desc g, const unsigned *__restrict__ d2, const double *__restrict__ sx,
                                                                 const double *__restrict__ sT, double margin, mpcmp_clearance *__restrict__ out,
                                                                 mpcmp_clearance_cert *__restrict__ cert) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag, n_level;
    const int b = blockIdx.x, tid = threadIdx.x, narm = h.narm, nseg = h.nseg, N = 3 * nseg + 1, nq = 7 * narm, nsph = h.ns0 + h.ns1;
    const int chunk = h.chunk, pitch = fcert_pitch(chunk), n_start = h.n_start, max_depth = h.max_depth;
    FcertLds L;
    MPCMP_FCERT_LAYOUT(L, lds, narm, nq, N, nsph, chunk)
    int *cur = L.cur, *nxt = L.nxt;

    if (tid == 0) nan_flag = 0;
    for (int e = tid; e < 84 * narm; e += CLR_NT) {
        const int a = e / 84, i = (e % 84) / 12, c = e % 12;
        L.mk[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    __syncthreads();
    const int n0 = nseg * n_start;
    const double *X = sx + (size_t)b * N * 2 * nq;
    for (int e = tid; e < nq * N; e += CLR_NT) {
        const double v = X[(size_t)(e / nq) * 2 * nq + e % nq];
        L.nodes[e] = v;
        if (!isfinite(v)) nan_flag = 1;
    }
    for (int s = tid; s < nsph; s += CLR_NT) {
        const ClrSphere S = sph[s];
        L.sk[4 * s] = S.c[0]; L.sk[4 * s + 1] = S.c[1]; L.sk[4 * s + 2] = S.c[2]; L.sk[4 * s + 3] = S.r;
        L.sj[s] = 7 * S.arm + S.joint; L.sa[s] = S.arm;
        cert_reach(L.mk + 84 * S.arm + 9, 12, S.joint, S.c, L.rch + 7 * s);
    }
    for (int e = tid; e < n0 && e < CERT_CAP; e += CLR_NT) cur[e] = e;
    __syncthreads();

    if (nan_flag) {                                      // (uniform)
        if (tid == 0) {
            out[b] = clr_nan_record();
            if (cert) cert[b] = cert_nan_record();
        }
        return;
    }

    CertBest B;                                          // (d, k: every thread; the rest: the deciding lanes only)
    int best_v = 0;                                      // the voxel read at B.d
    int n_cur = n0;
    for (int l = 0; n_cur > 0; l++) {
        B.depth = l;
        int n_split = 0;                                 // (uniform in the first wave)
        for (int c0 = 0; c0 < n_cur; c0 += chunk) {
            const int ns = (n_cur - c0 < chunk) ? n_cur - c0 : chunk;
            // A1
            for (int it = tid; it < ns * nq; it += CLR_NT) {
                const int sl = it / nq, j = it % nq;
                double qm;
                L.dv[it] = cert_deviation(L.nodes + j, nq, nseg, cert_interval(n0, n_start, l, cur[c0 + sl]), &qm);
                double sn, cs;
                sincos(qm, &sn, &cs);
                L.sc[2 * it] = sn; L.sc[2 * it + 1] = cs;
            }
            __syncthreads();
            // A2
            for (int it = tid; it < ns * narm; it += CLR_NT) {
                const int sl = it / narm, a = it % narm;
                cert_frames(L.mk + 84 * a, L.sc + (size_t)(sl * nq + 7 * a) * 2, L.fr + (size_t)(sl * nq + 7 * a) * 12);
            }
            __syncthreads();
            // B.  Every centre is finite (the nodes are, and so are sines and cosines), and fld_sd clamps it onto the grid: the gather stays inside
            // the field
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                const double *S = L.sk + 4 * s;
                double c[3];
                cert_centre(L.fr + (size_t)(sl * nq + L.sj[s]) * 12, S, c);
                int v;
                const double d = fcert_distance(g, d2, c, S[3], &v);
                const double D = cert_motion(L.rch + 7 * s, L.dv + sl * nq + 7 * L.sa[s]);
                L.pd[s * pitch + sl] = d; L.pl[s * pitch + sl] = d - D;
                const unsigned long long key = fcert_key(cert_tkey(l, cur[c0 + sl]), s);
                if (d < INFINITY && cert_better(d, key, B.d, B.k)) { B.d = d; B.k = key; best_v = v; }
            }
            __syncthreads();
            // D (chunk <= 64: the first wave decides; the other waves go on to the barrier that ends the chunk)
            if (tid < 64) {
                int what = -1, i = 0;
                double Lb = INFINITY;
                if (tid < ns) {
                    i = cur[c0 + tid];
                    double dmid = INFINITY;
                    for (int s = 0; s < nsph; s++) { dmid = fmin(dmid, L.pd[s * pitch + tid]); Lb = fmin(Lb, L.pl[s * pitch + tid]); }
                    what = cert_decide(dmid, Lb, margin, l, max_depth);
                }
                const unsigned long long want = __ballot(what == CERT_SPLIT_IT);
                if (what == CERT_SPLIT_IT) {
                    const int rank = n_split + __popcll(want & ((1ull << tid) - 1ull));
                    if (rank < CERT_SPLIT) { nxt[2 * rank] = 2 * i; nxt[2 * rank + 1] = 2 * i + 1; }
                    else what = CERT_UNDECIDED;          // (the capacity rule)
                }
                n_split += __popcll(want);
                if (n_split > CERT_SPLIT) n_split = CERT_SPLIT;
                if (what >= 0 && what != CERT_SPLIT_IT) {
                    const unsigned tkey = cert_tkey(l, i);
                    if (what == CERT_HIT) { B.n_hit++; if (tkey < B.first) B.first = tkey; }
                    else if (what == CERT_CLEAR) B.n_clear++;
                    else B.n_und++;
                    const unsigned long long lk = cert_key(tkey, 0, 0, 0);
                    if (cert_better(Lb, lk, B.L, B.Lk)) { B.L = Lb; B.Lk = lk; }
                }
                if (tid == 0) B.n_eval += ns;
            }
            __syncthreads();
        }
        if (tid == 0) n_level = 2 * n_split;
        __syncthreads();
        n_cur = n_level;
        int *sw = cur; cur = nxt; nxt = sw;
        __syncthreads();                                 // (n_level is written again only after every thread has read it)
    }

    // the deciding lanes: counts, the earliest hit and the best (L, key) over the first wave
    if (tid < 64) {
#pragma unroll
        for (int o2 = 32; o2 > 0; o2 >>= 1) {
            B.n_hit += __shfl_down(B.n_hit, o2); B.n_clear += __shfl_down(B.n_clear, o2); B.n_und += __shfl_down(B.n_und, o2);
            const unsigned of = __shfl_down(B.first, o2);
            if (of < B.first) B.first = of;
            const double ol = __shfl_down(B.L, o2);
            const unsigned long long olk = __shfl_down(B.Lk, o2);
            if (cert_better(ol, olk, B.L, B.Lk)) { B.L = ol; B.Lk = olk; }
        }
    }
    clr_reduce(B.d, B.k, &best_v);                       // (the voxel carried beside the key)
    if (tid == 0) {
        mpcmp_clearance r;
        mpcmp_clearance_cert c;
        const double Te = sT[b];
        cert_records(B, [&](unsigned tkey) { return cert_time(n0, tkey) * Te; }, &r, &c);
        if (B.k != CERT_NO_PAIR) r.other = best_v;
        out[b] = r;
        if (cert) cert[b] = c;
    }
}

// one lane per plan
__global__ __launch_bounds__(256) void k_clearance_cert_merge(int B, const mpcmp_clearance_cert *a, const mpcmp_clearance_cert *b,
                                                              mpcmp_clearance_cert *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    const mpcmp_clearance_cert r = fcert_merge(a[i], b[i]);      // (both read before the write: out may be a or b)
    out[i] = r;
}

hipError_t field_cert_prepare() {
    // the ceiling over every sphere count: two arms, 25 nodes
    const size_t mx = lds_ceiling([](int s) { return fcert_lds_bytes(FcertShape{2, 8, s, 0, fcert_chunk(2, s), 1, 0}); });
    return hipFuncSetAttribute((const void *)k_clearance_cert_field, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mx);
}

hipError_t clearance_cert_field_launch(const ClrTables &t, const FldArrays &f, int B, const double *d_sx, const double *d_sT, double margin, int n_start,
                                       int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st) {
    const int nsph = t.n_sph[0] + t.n_sph[1];
    const FcertShape h = {t.narm, t.nseg, t.n_sph[0], t.n_sph[1], fcert_chunk(t.narm, nsph), n_start, max_depth};
    hipLaunchKernelGGL(k_clearance_cert_field, dim3(B), dim3(CLR_NT), fcert_lds_bytes(h), st, t.d_model, h, t.d_sph, f.desc, f.d_d2, d_sx, d_sT, margin,
                       d_out, d_cert);
    return hipGetLastError();
}

hipError_t clearance_cert_merge_launch(int B, const mpcmp_clearance_cert *d_a, const mpcmp_clearance_cert *d_b, mpcmp_clearance_cert *d_out,
                                       hipStream_t st) {
    hipLaunchKernelGGL(k_clearance_cert_merge, dim3((B + 255) / 256), dim3(256), 0, st, B, d_a, d_b, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp
