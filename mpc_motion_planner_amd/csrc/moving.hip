// moving.hip — clearance in a world that moves (include/mpcmp_moving.h): the timed check k_clearance_timed, the start-delay search k_start_delay and
// the export of a plan's sphere centres as tracks, k_sphere_tracks.  A translation unit of its own, so that k_clearance and every other kernel
// compile exactly as before.  The rule's arithmetic is moving_rule.hpp, the frames and centres those of clearance_cert.hpp, the distance formulas
// and tie order those of clearance_rule.hpp: the host statements of model_host.cpp run the same source.
#include <hip/hip_runtime.h>
#include <cmath>
#include "moving.hpp"
#include "clearance_cert.hpp"
#include "plan_interp.hpp"

namespace mpcmp {

// One workgroup per plan, the shape of k_clearance: the tables staged in LDS once, then the samples in chunks of `chunk`, and per chunk
//   A0  one thread per sample: its place on the plan (the retimed clock of profile_place.hpp) and on the tracks' clock;
//   A1  one thread per (sample, joint): the node interpolant of the joint position and its sine / cosine;
//   A2  one thread per (sample, arm): the forward-kinematics chain;
//   B   one thread per (sample, sphere): world centre, then the obstacles, each shifted by its track's offset at the sample's world time;
//   C   one thread per (sample, sphere s): every partner sphere t > s that clr_pair admits.
// The tracks stay in global memory: a sample reads two keys per track, all lanes of a sample the same ones, and neighbouring samples neighbouring
// keys, so L2 serves them; 64 x 1024 keys would not fit beside the tables.
struct MvShape { int narm, nseg, n0, n1, n_obs, obs_stride, chunk; };
struct MvLds {
    double *mk, *nodes, *sk, *ok, *sc, *fr, *cen, *ss, *tt, *pf, *dly;
    unsigned long long *dk, *w0;
    int *sj, *sa, *ot, *tof, *lst, *hit, *pk, *pk1;
};
constexpr unsigned long long MV_KEY_INF = 0xFFF0000000000000ull;      // clr_tkey(+inf)
__device__ __forceinline__ double mv_unkey(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u));
}

__device__ __forceinline__ MvLds mv_carve(double *lds, const MvShape &h, int K) {
    const int N = 3 * h.nseg + 1, nq = 7 * h.narm, nsph = h.n0 + h.n1;
    MvLds L;
    L.mk = lds;                                              // [narm][7][12] = R0 (9), p (3)
    L.nodes = L.mk + 84 * h.narm;                            // [N][nq]
    L.sk = L.nodes + (size_t)nq * N;                         // [nsph][4] = c, r
    L.ok = L.sk + 4 * nsph;                                  // [n_obs][8]
    L.sc = L.ok + 8 * h.n_obs;                               // [chunk][nq][2]
    L.fr = L.sc + (size_t)h.chunk * nq * 2;                  // [chunk][nq][12] = Rw (9), pw (3)
    L.cen = L.fr + (size_t)h.chunk * nq * 12;                // [chunk][nsph][3]
    L.ss = L.cen + (size_t)h.chunk * nsph * 3;               // [chunk] normalised plan time
    L.tt = L.ss + h.chunk;                                   // [chunk] running time
    L.pf = L.tt + h.chunk;                                   // [chunk] weight of the later key
    L.dly = L.pf + h.chunk;                                  // [K]
    L.dk = reinterpret_cast<unsigned long long *>(L.dly + K);   // [K] ordered keys of the runs' minima over the tracked obstacles
    L.w0 = L.dk + K;                                         // [K] ... of the start posture at the world times delays[k]
    L.sj = reinterpret_cast<int *>(L.w0 + K);                // [nsph] arm * 7 + joint
    L.sa = L.sj + nsph;                                      // [nsph] arm
    L.ot = L.sa + nsph;                                      // [n_obs] type
    L.tof = L.ot + h.n_obs;                                  // [n_obs] track, -1: none
    L.lst = L.tof + h.n_obs;                                 // [n_obs] the tracked obstacles first, then the others (k_start_delay)
    L.hit = L.lst + h.n_obs;                                 // [chunk]
    L.pk = L.hit + h.chunk;                                  // [chunk] earlier key
    L.pk1 = L.pk + h.chunk;                                  // [chunk] later key
    return L;
}

// the tables of problem b into LDS; *nan_flag (LDS, cleared by the caller before a barrier) is set by a non-finite position node, sol_T, t_start or
// profile entry.  The caller's barrier follows
__device__ __forceinline__ void mv_stage(const MvLds &L, const MvShape &h, const mpcmp_model *__restrict__ mdl, const ClrSphere *__restrict__ sph,
                                         const mpcmp_obstacle *__restrict__ obs, const MvTracks &trk, const MvPlans &p, int b, int *nan_flag) {
    const int tid = threadIdx.x, N = 3 * h.nseg + 1, nq = 7 * h.narm, nsph = h.n0 + h.n1;
    for (int e = tid; e < 84 * h.narm; e += CLR_NT) {
        const int a = e / 84, i = (e % 84) / 12, c = e % 12;
        L.mk[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    const double *X = p.d_sx + (size_t)b * N * 2 * nq;
    bool bad = false;
    for (int e = tid; e < nq * N; e += CLR_NT) {
        const double v = X[(size_t)(e / nq) * 2 * nq + e % nq];
        L.nodes[e] = v;
        bad = bad || !mv_finite(v);
    }
    for (int s = tid; s < nsph; s += CLR_NT) {
        const ClrSphere S = sph[s];
        L.sk[4 * s] = S.c[0]; L.sk[4 * s + 1] = S.c[1]; L.sk[4 * s + 2] = S.c[2]; L.sk[4 * s + 3] = S.r;
        L.sj[s] = 7 * S.arm + S.joint; L.sa[s] = S.arm;
    }
    const mpcmp_obstacle *O = obs + (size_t)b * h.obs_stride;
    const int *TO = trk.n_tracks > 0 ? trk.d_track_of + (size_t)(h.obs_stride ? b : 0) * h.n_obs : nullptr;
    for (int o = tid; o < h.n_obs; o += CLR_NT) {
        clr_obs_prepare(O[o], L.ok + 8 * o);
        L.ot[o] = O[o].type;
        L.tof[o] = TO ? mv_track(TO[o], trk.n_tracks) : -1;
    }
    for (int e = tid; e < h.chunk; e += CLR_NT) L.hit[e] = 0;
    if (p.d_prof) {
        const double *pf = p.d_prof + (size_t)b * (p.n_grid + 1) * 2;
        for (int e = tid; e < 2 * (p.n_grid + 1); e += CLR_NT) bad = bad || !mv_finite(pf[e]);
    }
    if (tid == 0) bad = bad || !mv_finite(p.d_sT[b]) || (p.d_t_start && !mv_finite(p.d_t_start[b]));
    if (bad) *nan_flag = 1;
}

// phases A1 and A2 of a chunk of ns samples whose normalised times are in L.ss; ends with a barrier
__device__ __forceinline__ void mv_frames(const MvLds &L, const MvShape &h, int ns) {
    const int tid = threadIdx.x, nq = 7 * h.narm;
    for (int it = tid; it < ns * nq; it += CLR_NT) {
        const int sl = it / nq, j = it % nq;
        double Lg[4];
        const int s = mpcmp_plan::lagrange_segment(h.nseg, L.ss[sl], Lg);
        const double q = mpcmp_plan::interp_channel(L.nodes + j, nq, s, Lg);
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

// phase C of a chunk: the smallest robot-pair clearance of (sample sl, sphere s) and its partner
__device__ __forceinline__ double mv_pairs(const MvLds &L, int nsph, int sl, int s, int self_gap, int *tm) {
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

// the clearance of the centre (cx, cy, cz) of a sphere of radius r against obstacle o shifted by the offset of its track at the place w
__device__ __forceinline__ double mv_tracked(const MvLds &L, const double *__restrict__ off, int n_key, int o, const MvPlace &w, double cx, double cy,
                                             double cz, double r) {
    double p[3];
    mv_offset(off + (size_t)L.tof[o] * n_key * 3, w, p);
    return clr_sd(L.ot[o], L.ok + 8 * o, cx - p[0], cy - p[1], cz - p[2]) - r;
}

__global__ __launch_bounds__(CLR_NT) void k_clearance_timed(const mpcmp_model *__restrict__ mdl, MvShape h, int n_pts,
                                                            const ClrSphere *__restrict__ sph, const mpcmp_obstacle *__restrict__ obs, MvTracks trk,
                                                            MvPlans p, double margin, int self_gap, mpcmp_clearance *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red_d[CLR_NT / 64];
    __shared__ unsigned red_k[CLR_NT / 64];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    const MvLds L = mv_carve(lds, h, 0);
    if (tid == 0) nan_flag = 0;
    __syncthreads();
    mv_stage(L, h, mdl, sph, obs, trk, p, b, &nan_flag);
    __syncthreads();
    if (nan_flag) {                                          // (uniform: every thread reads the flag after the barrier)
        if (tid == 0) out[b] = mv_clearance_nan();
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
            cert_centre(L.fr + (size_t)(sl * 7 * h.narm + L.sj[s]) * 12, S, c);
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
                const double dm = mv_pairs(L, nsph, sl, s, self_gap, &tm);
                if (dm < margin) L.hit[sl] = 1;
                const unsigned k = clr_pack(ip0 + sl, s, 1, tm);
                if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; }
            }
            __syncthreads();
        }
        if (tid == 0)
            for (int sl = 0; sl < ns; sl++) {
                if (L.hit[sl]) { if (first < 0) first = ip0 + sl; n_hit++; }
                L.hit[sl] = 0;
            }
    }
    // workgroup reduction of (clearance, packed index) by clr_better
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
        const double od = __shfl_down(best_d, o2);
        const unsigned okk = __shfl_down(best_k, o2);
        if (clr_better(od, okk, best_d, best_k)) { best_d = od; best_k = okk; }
    }
    if ((tid & 63) == 0) { red_d[tid >> 6] = best_d; red_k[tid >> 6] = best_k; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CLR_NT / 64; w++)
            if (clr_better(red_d[w], red_k[w], best_d, best_k)) { best_d = red_d[w]; best_k = red_k[w]; }
        mpcmp_clearance r;
        r.d_min = best_d;
        if (best_k == CLR_NO_PAIR) { r.t_min = -1.0; r.sphere = -1; r.other = 0; }
        else {
            const int ip = (int)(best_k >> 17), idx = (int)(best_k & 0xFFu);
            r.t_min = ((double)ip / n_pts) * T_run;
            r.sphere = (int)((best_k >> 9) & 0x7Fu);
            r.other = (best_k & 0x100u) ? -1 - idx : idx;
        }
        r.t_first = first >= 0 ? ((double)first / n_pts) * T_run : -1.0;
        r.n_hit = n_hit;
        r.status = n_hit > 0 ? MPCMP_CLR_HIT : 0;
        out[b] = r;
    }
}

// The start-delay search: the robot's motion relative to its own start does not depend on the delay, so phases A0 - A2, the centres, the obstacles
// that stand still and the robot pairs run ONCE per sample and fold into one minimum per thread; only phase D, one thread per (sample, sphere,
// delay), reads the tracks.  The runs' minima are integer minima in LDS on the ordered key of clr_tkey: exact and order-independent.
__global__ __launch_bounds__(CLR_NT) void k_start_delay(const mpcmp_model *__restrict__ mdl, MvShape h, int n_pts, const ClrSphere *__restrict__ sph,
                                                        const mpcmp_obstacle *__restrict__ obs, MvTracks trk, MvPlans p, int K,
                                                        const double *__restrict__ delays, int check_wait, double margin, int self_gap,
                                                        double *__restrict__ d_min_all, mpcmp_start_delay *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red_d[CLR_NT / 64];
    __shared__ int nan_flag, n_trk;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    const MvLds L = mv_carve(lds, h, K);
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
            cert_centre(L.fr + (size_t)(sl * 7 * h.narm + L.sj[s]) * 12, S, c);
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
                best = fmin(best, mv_pairs(L, nsph, it / nsph, it % nsph, self_gap, &tm));
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
__global__ __launch_bounds__(CLR_NT) void k_sphere_tracks(const mpcmp_model *__restrict__ mdl, MvShape h, const ClrSphere *__restrict__ sph, MvPlans p,
                                                          double t0, double dt, int n_key, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    const MvLds L = mv_carve(lds, h, 0);
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
            cert_centre(L.fr + (size_t)(sl * 7 * h.narm + L.sj[s]) * 12, L.sk + 4 * s, c);
            double *W = O + ((size_t)s * n_key + k0 + sl) * 3;
            W[0] = c[0]; W[1] = c[1]; W[2] = c[2];
        }
        __syncthreads();
    }
}

static size_t mv_lds_ceiling(int K) {
    // as clearance_prepare: the ceiling over every sphere count (the chunk shrinks as the sphere tables grow), two arms, 25 nodes, 256 obstacles
    size_t mx = 0;
    for (int s = 0; s <= 2 * CLR_MAX_SPH; s++) {
        const size_t b = mv_lds_bytes(2, 25, s, CLR_MAX_OBS, clr_chunk(s), K);
        if (b > mx) mx = b;
    }
    return mx;
}

hipError_t moving_prepare() {
    hipError_t e = hipFuncSetAttribute((const void *)k_clearance_timed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(0));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void *)k_start_delay, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(MV_MAX_DELAYS));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)k_sphere_tracks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mv_lds_ceiling(0));
}

static MvShape mv_shape(const ClrTables &t, bool with_obs) {
    MvShape h;
    h.narm = t.narm; h.nseg = t.nseg; h.n0 = t.n_sph[0]; h.n1 = t.n_sph[1];
    h.n_obs = with_obs ? t.n_obs : 0; h.obs_stride = with_obs ? t.obs_stride : 0;
    h.chunk = clr_chunk(h.n0 + h.n1);
    return h;
}

hipError_t clearance_timed_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int n_pts, double margin, int self_gap,
                                  mpcmp_clearance *d_out, hipStream_t st) {
    const MvShape h = mv_shape(t, true);
    const size_t lds = mv_lds_bytes(h.narm, 3 * h.nseg + 1, h.n0 + h.n1, h.n_obs, h.chunk, 0);
    hipLaunchKernelGGL(k_clearance_timed, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, n_pts, t.d_sph, t.d_obs, trk, p, margin, self_gap, d_out);
    return hipGetLastError();
}

hipError_t start_delay_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int K, const double *d_delays, int check_wait,
                              int n_pts, double margin, int self_gap, double *d_min_all, mpcmp_start_delay *d_out, hipStream_t st) {
    const MvShape h = mv_shape(t, true);
    const size_t lds = mv_lds_bytes(h.narm, 3 * h.nseg + 1, h.n0 + h.n1, h.n_obs, h.chunk, K);
    hipLaunchKernelGGL(k_start_delay, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, n_pts, t.d_sph, t.d_obs, trk, p, K, d_delays, check_wait, margin,
                       self_gap, d_min_all, d_out);
    return hipGetLastError();
}

hipError_t sphere_tracks_launch(const ClrTables &t, const MvPlans &p, int B, double t0, double dt, int n_key, double *d_out, hipStream_t st) {
    const MvShape h = mv_shape(t, false);
    if (h.n0 + h.n1 < 1) return hipSuccess;
    const size_t lds = mv_lds_bytes(h.narm, 3 * h.nseg + 1, h.n0 + h.n1, 0, h.chunk, 0);
    hipLaunchKernelGGL(k_sphere_tracks, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, t.d_sph, p, t0, dt, n_key, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp
