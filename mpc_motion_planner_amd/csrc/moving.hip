// moving.hip — clearance in a world that moves (include/mpcmp_moving.h): the timed check k_clearance_timed, the start-delay search k_start_delay and
// the export of a plan's sphere centres as tracks, k_sphere_tracks.  A translation unit of its own, so that k_clearance and every other kernel
// compile exactly as before.  The rule's arithmetic is moving_rule.hpp, the frames and centres those of clearance_cert.hpp, the distance formulas
// and tie order those of clearance_rule.hpp: the host statements of model_host.cpp run the same source.
#include <hip/hip_runtime.h>
#include <cmath>
#include "moving.hpp"
#include "clearance_phases.hpp"

namespace mpcmp {

// One workgroup per plan, the shape of k_clearance: the tables staged in LDS once, then the samples in chunks of `chunk`, and per chunk
//   A0  one thread per sample: its place on the plan (the retimed clock of profile_place.hpp) and on the tracks' clock;
//   A1  one thread per (sample, joint): the node interpolant of the joint position and its sine / cosine;
//   A2  one thread per (sample, arm): the forward-kinematics chain;
//   B   one thread per (sample, sphere): world centre, then the obstacles, each shifted by its track's offset at the sample's world time;
//   C   one thread per (sample, sphere s): every partner sphere t > s that clr_pair admits.
// The tracks stay in global memory: a sample reads two keys per track, all lanes of a sample the same ones, and neighbouring samples neighbouring
// keys, so L2 serves them; 64 x 1024 keys would not fit beside the tables.
constexpr unsigned long long MV_KEY_INF = 0xFFF0000000000000ull;      // clr_tkey(+inf)
__device__ __forceinline__ double mv_unkey(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u));
}

// the tables of problem b into LDS (clr_stage) with the obstacles' tracks; *nan_flag (LDS, cleared by the caller before a barrier) is set by a
// non-finite position node, sol_T, t_start or profile entry: these kernels flag a NaN by the node.  The caller's barrier follows
__device__ __forceinline__ void mv_stage(const ClrLds &L, const ClrShape &h, const mpcmp_model *__restrict__ mdl, const ClrSphere *__restrict__ sph,
                                         const mpcmp_obstacle *__restrict__ obs, const MvTracks &trk, const MvPlans &p, int b, int *nan_flag) {
    const int tid = threadIdx.x;
    bool bad = clr_stage(L, h, mdl, sph, obs, p.d_sx, b);
    const int *TO = trk.n_tracks > 0 ? trk.d_track_of + (size_t)(h.obs_stride ? b : 0) * h.n_obs : nullptr;
    for (int o = tid; o < h.n_obs; o += CLR_NT) L.tof[o] = TO ? mv_track(TO[o], trk.n_tracks) : -1;
    if (p.d_prof) {
        const double *pf = p.d_prof + (size_t)b * (p.n_grid + 1) * 2;
        for (int e = tid; e < 2 * (p.n_grid + 1); e += CLR_NT) bad = bad || !mv_finite(pf[e]);
    }
    if (tid == 0) bad = bad || !mv_finite(p.d_sT[b]) || (p.d_t_start && !mv_finite(p.d_t_start[b]));
    if (bad) *nan_flag = 1;
}
// phases A1 and A2 of a chunk of ns samples whose normalised times are in L.ss; ends with a barrier
__device__ __forceinline__ void mv_frames(const ClrLds &L, const ClrShape &h, int ns) {
    clr_frames(L, h, ns, [&](int sl) { return L.ss[sl]; }, nullptr);
}

// the clearance of the centre (cx, cy, cz) of a sphere of radius r against obstacle o shifted by the offset of its track at the place w
__device__ __forceinline__ double mv_tracked(const ClrLds &L, const double *__restrict__ off, int n_key, int o, const MvPlace &w, double cx, double cy,
                                             double cz, double r) {
    double p[3];
    mv_offset(off + (size_t)L.tof[o] * n_key * 3, w, p);
    return clr_sd(L.ot[o], L.ok + 8 * o, cx - p[0], cy - p[1], cz - p[2]) - r;
}

__global__ __launch_bounds__(CLR_NT) void k_clearance_timed(const mpcmp_model *__restrict__ mdl, ClrShape h, int n_pts,
                                                            const ClrSphere *__restrict__ sph, const mpcmp_obstacle *__restrict__ obs, MvTracks trk,
                                                            MvPlans p, double margin, int self_gap, mpcmp_clearance *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    LdsCursor<true> cur = {reinterpret_cast<char *>(lds), 0};
    const ClrLds L = clr_carve(cur, h, CLR_LDS_TIMED, 0);
    if (tid == 0) nan_flag = 0;
    __syncthreads();
    mv_stage(L, h, mdl, sph, obs, trk, p, b, &nan_flag);
    __syncthreads();
    if (nan_flag) {                                          // (uniform: every thread reads the flag after the barrier)
        if (tid == 0) out[b] = clr_nan_record();
        return;
    }
    const double *pf = p.d_prof ? p.d_prof + (size_t)b * (p.n_grid + 1) * 2 : nullptr;
    const double T = p.d_sT[b], T_run = mv_run_time(pf, p.n_grid, T), ts = p.d_t_start ? p.d_t_start[b] : 0.0;
    const double *off = trk.n_tracks > 0 ? trk.d_offsets + (size_t)(h.obs_stride ? b : 0) * trk.n_tracks * trk.n_key * 3 : nullptr;

    double best_d = INFINITY;
    unsigned best_k = CLR_NO_PAIR;
    int n_hit = 0, first = -1;                               // (thread 0 only)
    const bool pairs = h.narm > 1 || self_gap > 0;
    for (int ip0 = 0; ip0 <= n_pts; ip0 += chunk) {
        const int ns = (n_pts + 1 - ip0 < chunk) ? n_pts + 1 - ip0 : chunk;
        // A0
        for (int sl = tid; sl < ns; sl += CLR_NT) {
            double t, s;
            mv_sample(pf, p.n_grid, T, T_run, ip0 + sl, n_pts, &t, &s);
            L.ss[sl] = s; L.tt[sl] = t;
            const MvPlace w = mv_place(trk.n_key, trk.t0, trk.dt, ts + t);
            L.pk[sl] = w.k; L.pk1[sl] = w.k1; L.pf[sl] = w.f;
        }
        __syncthreads();
        mv_frames(L, h, ns);
        // B
        for (int it = tid; it < ns * nsph; it += CLR_NT) {
            const int sl = it / nsph, s = it % nsph;
            const double *S = L.sk + 4 * s;
            double c[3];
            clr_centre(L, h, sl, s, c);
            L.cen[3 * it] = c[0]; L.cen[3 * it + 1] = c[1]; L.cen[3 * it + 2] = c[2];
            MvPlace w;
            w.k = L.pk[sl]; w.k1 = L.pk1[sl]; w.f = L.pf[sl];
            double dm = INFINITY;
            int om = 0;
            for (int o = 0; o < h.n_obs; o++) {
                const double d = L.tof[o] >= 0 ? mv_tracked(L, off, trk.n_key, o, w, c[0], c[1], c[2], S[3])
                                               : clr_sd(L.ot[o], L.ok + 8 * o, c[0], c[1], c[2]) - S[3];
                if (d < dm) { dm = d; om = o; }
            }
            if (dm < margin) L.hit[sl] = 1;
            const unsigned k = clr_pack(ip0 + sl, s, 0, om);
            if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; }
        }
        __syncthreads();
        // C
        if (pairs) {
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                int tm;
                const double dm = clr_pairs(L, nsph, sl, s, self_gap, &tm);
                if (dm < margin) L.hit[sl] = 1;
                const unsigned k = clr_pack(ip0 + sl, s, 1, tm);
                if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; }
            }
            __syncthreads();
        }
        if (tid == 0) clr_count_hits(L, ns, ip0, &first, &n_hit);
    }
    clr_reduce(best_d, best_k, nullptr);
    if (tid == 0) out[b] = clr_record(best_d, best_k, first, n_hit, n_pts, T_run);
}

// The start-delay search: the robot's motion relative to its own start does not depend on the delay, so phases A0 - A2, the centres, the obstacles
// that stand still and the robot pairs run ONCE per sample and fold into one minimum per thread; only phase D, one thread per (sample, sphere,
// delay), reads the tracks.  The runs' minima are integer minima in LDS on the ordered key of clr_tkey: exact and order-independent.
__global__ __launch_bounds__(CLR_NT) void k_start_delay(const mpcmp_model *__restrict__ mdl, ClrShape h, int n_pts, const ClrSphere *__restrict__ sph,
                                                        const mpcmp_obstacle *__restrict__ obs, MvTracks trk, MvPlans p, int K,
                                                        const double *__restrict__ delays, int check_wait, double margin, int self_gap,
                                                        double *__restrict__ d_min_all, mpcmp_start_delay *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red_d[CLR_NT / 64];
    __shared__ int nan_flag, n_trk;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    LdsCursor<true> cur = {reinterpret_cast<char *>(lds), 0};
    const ClrLds L = clr_carve(cur, h, CLR_LDS_TIMED, K);
    if (tid == 0) nan_flag = 0;
    __syncthreads();
    mv_stage(L, h, mdl, sph, obs, trk, p, b, &nan_flag);
    for (int k = tid; k < K; k += CLR_NT) {
        const double d = delays[k];
        L.dly[k] = d; L.dk[k] = MV_KEY_INF; L.w0[k] = MV_KEY_INF;
        if (!mv_finite(d)) nan_flag = 1;
    }
    __syncthreads();
    double *all = d_min_all ? d_min_all + (size_t)b * K : nullptr;
    if (nan_flag) {
        if (tid == 0) out[b] = mv_delay_nan(K, all);
        return;
    }
    if (tid == 0) {                                          // the tracked obstacles first, in table order, then the others
        int nt = 0;
        for (int o = 0; o < h.n_obs; o++) if (L.tof[o] >= 0) L.lst[nt++] = o;
        n_trk = nt;
        for (int o = 0; o < h.n_obs; o++) if (L.tof[o] < 0) L.lst[nt++] = o;
    }
    __syncthreads();
    const int nt = n_trk;
    const double *pf = p.d_prof ? p.d_prof + (size_t)b * (p.n_grid + 1) * 2 : nullptr;
    const double T = p.d_sT[b], T_run = mv_run_time(pf, p.n_grid, T);
    const double *off = trk.n_tracks > 0 ? trk.d_offsets + (size_t)(h.obs_stride ? b : 0) * trk.n_tracks * trk.n_key * 3 : nullptr;

    double best = INFINITY;                                  // over the obstacles that stand still and the robot pairs, all samples
    const bool pairs = h.narm > 1 || self_gap > 0;
    for (int ip0 = 0; ip0 <= n_pts; ip0 += chunk) {
        const int ns = (n_pts + 1 - ip0 < chunk) ? n_pts + 1 - ip0 : chunk;
        for (int sl = tid; sl < ns; sl += CLR_NT) {
            double t, s;
            mv_sample(pf, p.n_grid, T, T_run, ip0 + sl, n_pts, &t, &s);
            L.ss[sl] = s; L.tt[sl] = t;
        }
        __syncthreads();
        mv_frames(L, h, ns);
        for (int it = tid; it < ns * nsph; it += CLR_NT) {
            const int sl = it / nsph, s = it % nsph;
            const double *S = L.sk + 4 * s;
            double c[3];
            clr_centre(L, h, sl, s, c);
            L.cen[3 * it] = c[0]; L.cen[3 * it + 1] = c[1]; L.cen[3 * it + 2] = c[2];
            for (int e = nt; e < h.n_obs; e++) {
                const int o = L.lst[e];
                best = fmin(best, clr_sd(L.ot[o], L.ok + 8 * o, c[0], c[1], c[2]) - S[3]);
            }
        }
        __syncthreads();
        if (pairs)
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                int tm;
                best = fmin(best, clr_pairs(L, nsph, it / nsph, it % nsph, self_gap, &tm));
            }
        // D
        if (nt > 0)
            for (int it = tid; it < ns * nsph * K; it += CLR_NT) {
                const int k = it % K, r = it / K, s = r % nsph, sl = r / nsph;
                const double *C = L.cen + (size_t)r * 3;
                const MvPlace w = mv_place(trk.n_key, trk.t0, trk.dt, L.dly[k] + L.tt[sl]);
                double dm = INFINITY;
                for (int e = 0; e < nt; e++) dm = fmin(dm, mv_tracked(L, off, trk.n_key, L.lst[e], w, C[0], C[1], C[2], L.sk[4 * s + 3]));
                const unsigned long long key = clr_tkey(dm);
                if (key < L.dk[k]) atomicMin(L.dk + k, key);             // (the plain read only spares atomics: the slot never grows)
                if (ip0 + sl == 0 && key < L.w0[k]) atomicMin(L.w0 + k, key);
            }
        __syncthreads();
    }
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) best = fmin(best, __shfl_down(best, o2));
    if ((tid & 63) == 0) red_d[tid >> 6] = best;
    __syncthreads();
    for (int w = 1; w < CLR_NT / 64; w++) best = fmin(best, red_d[w]);      // (thread 0 holds the workgroup's minimum now)
    if (tid == 0) {
        // the keys back to doubles in their own slots, each run joined with what does not depend on the delay
        double *dk = reinterpret_cast<double *>(L.dk), *w0 = reinterpret_cast<double *>(L.w0);
        for (int k = 0; k < K; k++) {
            const double a = mv_unkey(L.dk[k]), c = mv_unkey(L.w0[k]);
            dk[k] = fmin(a, best); w0[k] = c;
        }
        out[b] = mv_delay_record(K, L.dly, dk, w0, check_wait, margin, all);
    }
}

// the world centres of the robot spheres at the world times t0 + k dt: phases A0 - A2 and the centre part of B, written out as a track table
__global__ __launch_bounds__(CLR_NT) void k_sphere_tracks(const mpcmp_model *__restrict__ mdl, ClrShape h, const ClrSphere *__restrict__ sph, MvPlans p,
                                                          double t0, double dt, int n_key, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    LdsCursor<true> cur = {reinterpret_cast<char *>(lds), 0};
    const ClrLds L = clr_carve(cur, h, CLR_LDS_TIMED, 0);
    if (tid == 0) nan_flag = 0;
    __syncthreads();
    MvTracks none;
    none.d_track_of = nullptr; none.d_offsets = nullptr; none.n_tracks = 0; none.n_key = 1; none.t0 = 0.0; none.dt = 1.0;
    mv_stage(L, h, mdl, sph, nullptr, none, p, b, &nan_flag);            // (h.n_obs == 0 here: no obstacle is read)
    __syncthreads();
    double *O = out + (size_t)b * nsph * n_key * 3;
    if (nan_flag) {
        for (int e = tid; e < nsph * n_key * 3; e += CLR_NT) O[e] = NAN;
        return;
    }
    const double *pf = p.d_prof ? p.d_prof + (size_t)b * (p.n_grid + 1) * 2 : nullptr;
    const double T = p.d_sT[b], T_run = mv_run_time(pf, p.n_grid, T), ts = p.d_t_start ? p.d_t_start[b] : 0.0;
    for (int k0 = 0; k0 < n_key; k0 += chunk) {
        const int ns = (n_key - k0 < chunk) ? n_key - k0 : chunk;
        for (int sl = tid; sl < ns; sl += CLR_NT) L.ss[sl] = mv_held_s(pf, p.n_grid, T, T_run, t0 + (k0 + sl) * dt - ts);
        __syncthreads();
        mv_frames(L, h, ns);
        for (int it = tid; it < ns * nsph; it += CLR_NT) {
            const int sl = it / nsph, s = it % nsph;
            double c[3];
            clr_centre(L, h, sl, s, c);
            double *W = O + ((size_t)s * n_key + k0 + sl) * 3;
            W[0] = c[0]; W[1] = c[1]; W[2] = c[2];
        }
        __syncthreads();
    }
}

static size_t mv_lds_ceiling(int K) {
    // as clearance_prepare: two arms, 25 nodes, 256 obstacles
    return lds_ceiling([K](int s) { return clr_lds_bytes(ClrShape{2, 8, s, 0, CLR_MAX_OBS, 0, clr_chunk(s)}, CLR_LDS_TIMED, K); });
}

hipError_t moving_prepare() {
    hipError_t e = hipFuncSetAttribute((const void *)k_clearance_timed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(0));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void *)k_start_delay, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(MV_MAX_DELAYS));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)k_sphere_tracks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(0));
}

hipError_t clearance_timed_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int n_pts, double margin, int self_gap,
                                  mpcmp_clearance *d_out, hipStream_t st) {
    const ClrShape h = clr_shape(t, true);
    const size_t lds = clr_lds_bytes(h, CLR_LDS_TIMED, 0);
    hipLaunchKernelGGL(k_clearance_timed, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, n_pts, t.d_sph, t.d_obs, trk, p, margin, self_gap, d_out);
    return hipGetLastError();
}

hipError_t start_delay_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int K, const double *d_delays, int check_wait,
                              int n_pts, double margin, int self_gap, double *d_min_all, mpcmp_start_delay *d_out, hipStream_t st) {
    const ClrShape h = clr_shape(t, true);
    const size_t lds = clr_lds_bytes(h, CLR_LDS_TIMED, K);
    hipLaunchKernelGGL(k_start_delay, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, n_pts, t.d_sph, t.d_obs, trk, p, K, d_delays, check_wait, margin,
                       self_gap, d_min_all, d_out);
    return hipGetLastError();
}

hipError_t sphere_tracks_launch(const ClrTables &t, const MvPlans &p, int B, double t0, double dt, int n_key, double *d_out, hipStream_t st) {
    const ClrShape h = clr_shape(t, false);
    if (h.n0 + h.n1 < 1) return hipSuccess;
    const size_t lds = clr_lds_bytes(h, CLR_LDS_TIMED, 0);
    hipLaunchKernelGGL(k_sphere_tracks, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, t.d_sph, p, t0, dt, n_key, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp
