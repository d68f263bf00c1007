// moving_cert.hip — the kernel of the certified check in a moving world (include/mpcmp_moving_cert.h; the rule is moving_cert_rule.hpp on top of
// clearance_cert.hpp and moving_rule.hpp, which the host statement in model_host.cpp runs as well).  A translation unit of its own, so that
// k_clearance_cert, the kernels of moving.hip and every other unit compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "moving_cert.hpp"
#include "moving_cert_rule.hpp"

namespace mpcmp {

// intervals per chunk: the rule of k_clearance_cert (chunk x spheres <= 512 per-sphere records in LDS, at most 16: one lane of the first wave each)
static inline int mvc_chunk(int nsph) {
    const int c = nsph > 0 ? 512 / nsph : 16;
    return c > 16 ? 16 : (c < 1 ? 1 : c);
}
// dynamic LDS of k_clearance_cert_timed in bytes: what k_clearance_cert holds, the chunk's track table (p_m, E_k per interval and track) and the
// obstacles' tracks; it does not depend on n_start, n_rest or max_depth
static inline size_t mvc_lds_bytes(int narm, int N, int nsph, int n_obs, int n_tracks, int chunk) {
    const size_t dbl = (size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)7 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 21 +
                       (size_t)chunk * narm * 84 + (size_t)chunk * nsph * 6 + (size_t)chunk * n_tracks * 4;
    const size_t ints = (size_t)2 * CERT_CAP + (size_t)2 * nsph + (size_t)2 * n_obs;
    return dbl * sizeof(double) + (ints + 1) / 2 * 2 * sizeof(int);
}

struct MvcShape { int narm, nseg, ns0, ns1, n_obs, obs_stride, chunk, n_start, n_rest, max_depth; };

// One workgroup per plan: k_clearance_cert with a timeline.  Staged in LDS once: the joint placements, the position nodes, the sphere tables with
// their reach, the problem's obstacles and their tracks' indices.  Two lists of GLOBAL interval indices in LDS, the current level's and the next
// one's, both in time order; an interval's phase (wait, motion, hold) follows from its index (mvc_interval).  A level runs in chunks of `chunk`
// intervals, six phases per chunk:
//   T   one thread per (interval, track of the problem's set): p_m and E_k (mvc_track_bound) into LDS; the key loop runs over the keys inside the
//       interval only, so it is short below level 0.  The tracks stay in global memory, as in k_clearance_timed;
//   A1  one thread per (interval, joint): q(t_m) with its sine / cosine, and dev; a rest interval reads its node and has dev = 0 (no Bezier work);
//   A2  one thread per (interval, arm): the frames of the arm at t_m;
//   B   one thread per (interval, sphere): D_s, the world centre, then every obstacle (a uniform loop: all lanes look at the same obstacle, hence the
//       same track): the smallest d, and the smallest bound d - D_s - E_k, which the tracks make a minimum of its own;
//   C   one thread per (interval, sphere s): every partner t > s that clr_pair admits, d and d - D_s - D_t;
//   D   one lane of the first wave per interval: the minima over the spheres, the decision, and the children appended to the next list at the rank
//       a ballot gives them.
// Every thread keeps its best (d, key) in registers over all chunks and levels, the deciding lanes their leaf counts and best (L, key); one
// reduction at the end, ordered by the keys, so the records do not depend on the launch or on the batch.  No atomics.
__global__ __launch_bounds__(CLR_NT) void k_clearance_cert_timed(const mpcmp_model *__restrict__ mdl, MvcShape h, const ClrSphere *__restrict__ sph,
                                                                 const mpcmp_obstacle *__restrict__ obs, MvTracks trk, MvcPlans p, double margin,
                                                                 int self_gap, mpcmp_clearance *__restrict__ out,
                                                                 mpcmp_clearance_cert *__restrict__ cert) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red_d[CLR_NT / 64];
    __shared__ unsigned long long red_k[CLR_NT / 64];
    __shared__ int nan_flag, n_level;
    const int b = blockIdx.x, tid = threadIdx.x, narm = h.narm, nseg = h.nseg, N = 3 * nseg + 1, nq = 7 * narm, nsph = h.ns0 + h.ns1;
    const int n_obs = h.n_obs, chunk = h.chunk, n_start = h.n_start, max_depth = h.max_depth, n_tracks = trk.n_tracks, n_key = trk.n_key;
    double *mk_ = lds;                                   // [narm][7][12] = R0 (9), p (3)
    double *nodes = mk_ + 84 * narm;                     // [N][nq]
    double *sk = nodes + (size_t)nq * N;                 // [nsph][4] = c, r
    double *rch = sk + 4 * nsph;                         // [nsph][7]
    double *ok = rch + 7 * nsph;                         // [n_obs][8]
    double *sc = ok + 8 * n_obs;                         // [chunk][nq][2]
    double *dv = sc + (size_t)chunk * nq * 2;            // [chunk][nq]
    double *fr = dv + (size_t)chunk * nq;                // [chunk][nq][12] = Rw (9), pw (3)
    double *cen = fr + (size_t)chunk * nq * 12;          // [chunk][nsph][3]
    double *Dl = cen + (size_t)chunk * nsph * 3;         // [chunk][nsph] D_s
    double *pd = Dl + (size_t)chunk * nsph;              // [chunk][nsph] smallest d of the sphere's pairs
    double *pl = pd + (size_t)chunk * nsph;              // [chunk][nsph] smallest bound of the sphere's pairs
    double *tk = pl + (size_t)chunk * nsph;              // [chunk][n_tracks][4] = p_m (3), E_k
    int *cur = reinterpret_cast<int *>(tk + (size_t)chunk * n_tracks * 4);       // [CERT_CAP]
    int *nxt = cur + CERT_CAP;                           // [CERT_CAP]
    int *sj = nxt + CERT_CAP;                            // [nsph] arm * 7 + joint
    int *sa = sj + nsph;                                 // [nsph] arm
    int *ot = sa + nsph;                                 // [n_obs] type
    int *tof = ot + n_obs;                               // [n_obs] track, -1: none

    const double T = p.d_sT[b], ts = p.d_t_start ? p.d_t_start[b] : 0.0, w = p.d_wait ? p.d_wait[b] : 0.0, hd = p.d_hold ? p.d_hold[b] : 0.0;
    if (tid == 0) nan_flag = mvc_times_ok(T, ts, w, hd) ? 0 : 1;
    for (int e = tid; e < 84 * narm; e += CLR_NT) {
        const int a = e / 84, i = (e % 84) / 12, c = e % 12;
        mk_[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    __syncthreads();
    // (an invalid time may leave n0 anywhere: the lists are filled only behind the flag)
    const MvcTimeline tl = mvc_timeline(nseg, n_start, h.n_rest, T, ts, w, hd);
    const int n0 = tl.n0;
    const double *X = p.d_sx + (size_t)b * N * 2 * nq;
    for (int e = tid; e < nq * N; e += CLR_NT) {
        const double v = X[(size_t)(e / nq) * 2 * nq + e % nq];
        nodes[e] = v;
        if (!mv_finite(v)) nan_flag = 1;
    }
    for (int s = tid; s < nsph; s += CLR_NT) {
        const ClrSphere S = sph[s];
        sk[4 * s] = S.c[0]; sk[4 * s + 1] = S.c[1]; sk[4 * s + 2] = S.c[2]; sk[4 * s + 3] = S.r;
        sj[s] = 7 * S.arm + S.joint; sa[s] = S.arm;
        cert_reach(mk_ + 84 * S.arm + 9, 12, S.joint, S.c, rch + 7 * s);
    }
    const mpcmp_obstacle *O = obs + (size_t)b * h.obs_stride;
    const int *TO = n_tracks > 0 ? trk.d_track_of + (size_t)(h.obs_stride ? b : 0) * n_obs : nullptr;
    for (int o = tid; o < n_obs; o += CLR_NT) {
        clr_obs_prepare(O[o], ok + 8 * o);
        ot[o] = O[o].type;
        tof[o] = TO ? mv_track(TO[o], n_tracks) : -1;
    }
    for (int e = tid; e < n0 && e < CERT_CAP; e += CLR_NT) cur[e] = e;
    __syncthreads();

    if (nan_flag) {                                      // (uniform)
        if (tid == 0) {
            out[b] = mv_clearance_nan();
            if (cert) {
                mpcmp_clearance_cert c;
                c.d_lower = NAN; c.t_lower = -1.0; c.n_eval = 0; c.n_clear = 0; c.n_undecided = 0; c.depth = 0;
                cert[b] = c;
            }
        }
        return;
    }
    const double *off = n_tracks > 0 ? trk.d_offsets + (size_t)(h.obs_stride ? b : 0) * n_tracks * n_key * 3 : nullptr;

    double best_d = INFINITY, best_L = INFINITY;
    unsigned long long best_k = CERT_NO_PAIR, best_Lk = CERT_NO_PAIR;
    unsigned first = CERT_NO_TIME;                       // (the deciding lanes only, as the counts)
    int n_hit = 0, n_clear = 0, n_und = 0, n_eval = 0, depth = 0;
    const bool pairs = narm > 1 || self_gap > 0;
    int n_cur = n0;
    for (int l = 0; n_cur > 0; l++) {
        depth = l;
        int n_split = 0;                                 // (uniform in the first wave)
        for (int c0 = 0; c0 < n_cur; c0 += chunk) {
            const int ns = (n_cur - c0 < chunk) ? n_cur - c0 : chunk;
            // T
            for (int it = tid; it < ns * n_tracks; it += CLR_NT) {
                const int sl = it / n_tracks, k = it % n_tracks;
                const MvcInterval v = mvc_interval(tl, n_start, l, cur[c0 + sl]);
                double pm[3];
                const double E = mvc_track_bound(off + (size_t)k * n_key * 3, n_key, trk.t0, trk.dt, tl.tau0 + v.ta, tl.tau0 + v.tm, tl.tau0 + v.tb, pm);
                tk[4 * it] = pm[0]; tk[4 * it + 1] = pm[1]; tk[4 * it + 2] = pm[2]; tk[4 * it + 3] = E;
            }
            // A1
            for (int it = tid; it < ns * nq; it += CLR_NT) {
                const int sl = it / nq, j = it % nq;
                const MvcInterval v = mvc_interval(tl, n_start, l, cur[c0 + sl]);
                double qm, dev = 0.0;
                if (v.phase == MVC_MOTION) dev = cert_deviation(nodes + j, nq, nseg, v.v, &qm);
                else qm = nodes[(v.phase == MVC_HOLD ? (N - 1) * nq : 0) + j];
                dv[it] = dev;
                double sn, cs;
                sincos(qm, &sn, &cs);
                sc[2 * it] = sn; sc[2 * it + 1] = cs;
            }
            __syncthreads();
            // A2
            for (int it = tid; it < ns * narm; it += CLR_NT) {
                const int sl = it / narm, a = it % narm;
                cert_frames(mk_ + 84 * a, sc + (size_t)(sl * nq + 7 * a) * 2, fr + (size_t)(sl * nq + 7 * a) * 12);
            }
            __syncthreads();
            // B
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                const double *S = sk + 4 * s;
                const double D = cert_motion(rch + 7 * s, dv + sl * nq + 7 * sa[s]);
                double c[3];
                cert_centre(fr + (size_t)(sl * nq + sj[s]) * 12, S, c);
                cen[3 * it] = c[0]; cen[3 * it + 1] = c[1]; cen[3 * it + 2] = c[2];
                const double *TK = tk + (size_t)sl * n_tracks * 4;
                double dm = INFINITY, lm = INFINITY;
                int om = 0;
                for (int o = 0; o < n_obs; o++) {
                    const int k = tof[o];
                    double d, bound;
                    if (k >= 0) {
                        const double *M = TK + 4 * k;
                        d = clr_sd(ot[o], ok + 8 * o, c[0] - M[0], c[1] - M[1], c[2] - M[2]) - S[3];
                        bound = d - D - M[3];
                    } else {
                        d = clr_sd(ot[o], ok + 8 * o, c[0], c[1], c[2]) - S[3];
                        bound = d - D;
                    }
                    if (d < dm) { dm = d; om = o; }
                    lm = fmin(lm, bound);
                }
                Dl[it] = D; pd[it] = dm; pl[it] = lm;
                const unsigned long long key = cert_key(cert_tkey(l, cur[c0 + sl]), s, 0, om);
                if (dm < INFINITY && cert_better(dm, key, best_d, best_k)) { best_d = dm; best_k = key; }
            }
            __syncthreads();
            // C
            if (pairs) {
                for (int it = tid; it < ns * nsph; it += CLR_NT) {
                    const int sl = it / nsph, s = it % nsph;
                    const double *C = cen + (size_t)sl * nsph * 3, *DD = Dl + (size_t)sl * nsph;
                    const double cx = C[3 * s], cy = C[3 * s + 1], cz = C[3 * s + 2], rs = sk[4 * s + 3], Dsv = DD[s];
                    const int as = sa[s], js = sj[s];
                    double dm = INFINITY, lm = INFINITY;
                    int tm = 0;
                    for (int t = s + 1; t < nsph; t++) {
                        if (!clr_pair(as, js, sa[t], sj[t], self_gap)) continue;      // (sj holds arm * 7 + joint: differences within one arm are joint differences)
                        const double ex = cx - C[3 * t], ey = cy - C[3 * t + 1], ez = cz - C[3 * t + 2];
                        const double d = sqrt(ex * ex + ey * ey + ez * ez) - rs - sk[4 * t + 3];
                        if (d < dm) { dm = d; tm = t; }
                        lm = fmin(lm, d - Dsv - DD[t]);
                    }
                    pd[it] = fmin(pd[it], dm); pl[it] = fmin(pl[it], lm);
                    const unsigned long long key = cert_key(cert_tkey(l, cur[c0 + sl]), s, 1, tm);
                    if (dm < INFINITY && cert_better(dm, key, best_d, best_k)) { best_d = dm; best_k = key; }
                }
                __syncthreads();
            }
            // D (chunk <= 16: the first wave decides; the other waves go on to the barrier that ends the chunk)
            if (tid < 64) {
                int what = -1, i = 0;
                double L = INFINITY;
                if (tid < ns) {
                    i = cur[c0 + tid];
                    double dmid = INFINITY;
                    for (int s = 0; s < nsph; s++) { dmid = fmin(dmid, pd[tid * nsph + s]); L = fmin(L, pl[tid * nsph + s]); }
                    what = cert_decide(dmid, L, margin, l, max_depth);
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
                    if (what == CERT_HIT) { n_hit++; if (tkey < first) first = tkey; }
                    else if (what == CERT_CLEAR) n_clear++;
                    else n_und++;
                    const unsigned long long lk = cert_key(tkey, 0, 0, 0);
                    if (cert_better(L, lk, best_L, best_Lk)) { best_L = L; best_Lk = lk; }
                }
                if (tid == 0) n_eval += ns;
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
            n_hit += __shfl_down(n_hit, o2); n_clear += __shfl_down(n_clear, o2); n_und += __shfl_down(n_und, o2);
            const unsigned of = __shfl_down(first, o2);
            if (of < first) first = of;
            const double ol = __shfl_down(best_L, o2);
            const unsigned long long olk = __shfl_down(best_Lk, o2);
            if (cert_better(ol, olk, best_L, best_Lk)) { best_L = ol; best_Lk = olk; }
        }
    }
    // workgroup reduction of (clearance, key) by cert_better
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) {
        const double od = __shfl_down(best_d, o2);
        const unsigned long long okk = __shfl_down(best_k, o2);
        if (cert_better(od, okk, best_d, best_k)) { best_d = od; best_k = okk; }
    }
    if ((tid & 63) == 0) { red_d[tid >> 6] = best_d; red_k[tid >> 6] = best_k; }
    __syncthreads();
    if (tid == 0) {
        for (int wv = 1; wv < CLR_NT / 64; wv++)
            if (cert_better(red_d[wv], red_k[wv], best_d, best_k)) { best_d = red_d[wv]; best_k = red_k[wv]; }
        mpcmp_clearance r;
        r.d_min = best_d;
        if (best_k == CERT_NO_PAIR) { r.t_min = -1.0; r.sphere = -1; r.other = 0; }
        else {
            const int idx = (int)(best_k & 0xFFu);
            r.t_min = mvc_time(tl, (unsigned)(best_k >> 16));
            r.sphere = (int)((best_k >> 9) & 0x7Fu);
            r.other = (best_k & 0x100u) ? -1 - idx : idx;
        }
        r.t_first = first != CERT_NO_TIME ? mvc_time(tl, first) : -1.0;
        r.n_hit = n_hit;
        r.status = (n_hit > 0 ? MPCMP_CLR_HIT : 0) | (n_und > 0 ? MPCMP_CLR_UNDECIDED : 0);
        out[b] = r;
        if (cert) {
            mpcmp_clearance_cert c;
            c.d_lower = best_L; c.t_lower = mvc_time(tl, (unsigned)(best_Lk >> 16));
            c.n_eval = n_eval; c.n_clear = n_clear; c.n_undecided = n_und; c.depth = depth;
            cert[b] = c;
        }
    }
}

hipError_t moving_cert_prepare() {
    // the ceiling over every sphere count (the chunk shrinks as the sphere tables grow), two arms, 25 nodes, 256 obstacles, 64 tracks
    size_t mx = 0;
    for (int s = 0; s <= 2 * CLR_MAX_SPH; s++) {
        const size_t b = mvc_lds_bytes(2, 25, s, CLR_MAX_OBS, MV_MAX_TRACKS, mvc_chunk(s));
        if (b > mx) mx = b;
    }
    return hipFuncSetAttribute((const void *)k_clearance_cert_timed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mx);
}

hipError_t moving_cert_launch(const ClrTables &t, const MvTracks &trk, const MvcPlans &p, int B, double margin, int self_gap, int n_start, int n_rest,
                              int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st) {
    MvcShape h;
    h.narm = t.narm; h.nseg = t.nseg; h.ns0 = t.n_sph[0]; h.ns1 = t.n_sph[1]; h.n_obs = t.n_obs; h.obs_stride = t.obs_stride;
    h.chunk = mvc_chunk(h.ns0 + h.ns1); h.n_start = n_start; h.n_rest = n_rest; h.max_depth = max_depth;
    const size_t lds = mvc_lds_bytes(h.narm, 3 * h.nseg + 1, h.ns0 + h.ns1, h.n_obs, trk.n_tracks, h.chunk);
    hipLaunchKernelGGL(k_clearance_cert_timed, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, t.d_sph, t.d_obs, trk, p, margin, self_gap, d_out, d_cert);
    return hipGetLastError();
}

}  // namespace mpcmp
