// clearance_cert.hip — the kernel of the certified clearance check, without a timeline (include/mpcmp_clearance_cert.h) and with one
// (include/mpcmp_moving_cert.h): one text (cert_search), two kernels.  The rule is clearance_cert.hpp and, for the timeline, moving_cert_rule.hpp, which
// the host statements in model_host.cpp run as well.  A translation unit of its own, so that every other unit compiles exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "moving.hpp"
#include "moving_cert_rule.hpp"
#include "clearance_phases.hpp"

namespace mpcmp {

// One workgroup per plan.  Staged in LDS once: the joint placements, the position nodes, the sphere tables with their reach, the problem's
// obstacles.  Two lists of interval indices in LDS, the current level's and the next one's, both in time order.  A level runs in chunks of `chunk`
// intervals, five phases per chunk:
//   A1  one thread per (interval, joint): q(t_m) with its sine / cosine, and dev (cert_deviation);
//   A2  one thread per (interval, arm): the frames of the arm at t_m (cert_frames), once per interval;
//   B   one thread per (interval, sphere): D_s, the world centre, then every obstacle (a uniform loop, broadcast reads): the smallest d and the
//       smallest bound;
//   C   one thread per (interval, sphere s): every partner t > s that clr_pair admits, d and d - D_s - D_t;
//   D   one lane of the first wave per interval: the minima over the spheres, the decision, and the children of the intervals to be split appended
//       to the next list at the rank a ballot gives them: time order and the capacity rule without a counter that threads race for.
// Every thread keeps its best (d, key) in registers over all chunks and levels, the deciding lanes their leaf counts and best (L, key); one
// reduction at the end, ordered by the keys, so the records do not depend on the launch or on the batch.  No atomics.
//
// TL: with a timeline (cert_search<true> = k_clearance_cert_timed, the check in a moving world).  The interval indices are then GLOBAL over wait, motion and hold, an
// interval's phase follows from its index (mvc_interval), a rest interval reads its node and has dev = 0, the obstacles' tracks are staged beside
// their types, and a sixth phase comes first in a chunk:
//   T   one thread per (interval, track of the problem's set): p_m and E_k (mvc_track_bound) into LDS; the key loop runs over the keys inside the
//       interval only, so it is short below level 0.  The tracks stay in global memory, as in k_clearance_timed.
// Without one (cert_search<false> = k_clearance_cert, the static certificate) phase T, the tracks with their LDS, the rest branches and the check of the times are
// compiled out: trk and the rests of p are not read, so the obstacles stand where mpcmp_set_obstacles put them whatever tracks the context holds,
// and sol_T is not tested (a non-finite one only makes the times non-finite).
template <bool TL>
__device__ __forceinline__ void cert_search(const mpcmp_model *__restrict__ mdl, const CertShape &h, const ClrSphere *__restrict__ sph,
                                            const mpcmp_obstacle *__restrict__ obs, const MvTracks &trk, const CertPlans &p, double margin, int self_gap,
                                            mpcmp_clearance *__restrict__ out, mpcmp_clearance_cert *__restrict__ cert) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag, n_level;
    const int b = blockIdx.x, tid = threadIdx.x, narm = h.narm, nseg = h.nseg, N = 3 * nseg + 1, nq = 7 * narm, nsph = h.ns0 + h.ns1;
    const int n_obs = h.n_obs, obs_stride = h.obs_stride, chunk = h.chunk, n_start = h.n_start, max_depth = h.max_depth;
    const int n_tracks = TL ? trk.n_tracks : 0, n_key = TL ? trk.n_key : 1;
    CertLds L;
    MPCMP_CERT_LAYOUT(L, lds, narm, nq, N, nsph, n_obs, chunk, TL, n_tracks)
    int *cur = L.cur, *nxt = L.nxt;

    double T = 0.0, ts = 0.0, w = 0.0, hd = 0.0;         // (the static certificate reads sol_T at the end only)
    if (TL) { T = p.d_sT[b]; ts = p.d_t_start ? p.d_t_start[b] : 0.0; w = p.d_wait ? p.d_wait[b] : 0.0; hd = p.d_hold ? p.d_hold[b] : 0.0; }
    if (tid == 0) nan_flag = (!TL || mvc_times_ok(T, ts, w, hd)) ? 0 : 1;
    for (int e = tid; e < 84 * narm; e += CLR_NT) {
        const int a = e / 84, i = (e % 84) / 12, c = e % 12;
        L.mk[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    __syncthreads();
    // (with a timeline an invalid time may leave n0 anywhere: the lists are filled only behind the flag)
    MvcTimeline tl;
    if (TL) tl = mvc_timeline(nseg, n_start, h.n_rest, T, ts, w, hd);
    const int n0 = TL ? tl.n0 : nseg * n_start;
    const double *X = p.d_sx + (size_t)b * N * 2 * nq;
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
    const mpcmp_obstacle *O = obs + (size_t)b * obs_stride;
    const int *TO = n_tracks > 0 ? trk.d_track_of + (size_t)(obs_stride ? b : 0) * n_obs : nullptr;
    for (int o = tid; o < n_obs; o += CLR_NT) {
        clr_obs_prepare(O[o], L.ok + 8 * o);
        L.ot[o] = O[o].type;
        if (TL) L.tof[o] = TO ? mv_track(TO[o], n_tracks) : -1;
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
    const double *off = n_tracks > 0 ? trk.d_offsets + (size_t)(obs_stride ? b : 0) * n_tracks * n_key * 3 : nullptr;

    CertBest B;                                          // (d, k: every thread; the rest: the deciding lanes only)
    const bool pairs = narm > 1 || self_gap > 0;
    int n_cur = n0;
    for (int l = 0; n_cur > 0; l++) {
        B.depth = l;
        int n_split = 0;                                 // (uniform in the first wave)
        for (int c0 = 0; c0 < n_cur; c0 += chunk) {
            const int ns = (n_cur - c0 < chunk) ? n_cur - c0 : chunk;
            // T
            if (TL)
                for (int it = tid; it < ns * n_tracks; it += CLR_NT) {
                    const int sl = it / n_tracks, k = it % n_tracks;
                    const MvcInterval v = mvc_interval(tl, n_start, l, cur[c0 + sl]);
                    double pm[3];
                    const double E = mvc_track_bound(off + (size_t)k * n_key * 3, n_key, trk.t0, trk.dt, tl.tau0 + v.ta, tl.tau0 + v.tm, tl.tau0 + v.tb, pm);
                    L.tk[4 * it] = pm[0]; L.tk[4 * it + 1] = pm[1]; L.tk[4 * it + 2] = pm[2]; L.tk[4 * it + 3] = E;
                }
            // A1
            for (int it = tid; it < ns * nq; it += CLR_NT) {
                const int sl = it / nq, j = it % nq;
                double qm, dev = 0.0;
                if (TL) {
                    const MvcInterval v = mvc_interval(tl, n_start, l, cur[c0 + sl]);
                    if (v.phase == MVC_MOTION) dev = cert_deviation(L.nodes + j, nq, nseg, v.v, &qm);
                    else qm = L.nodes[(v.phase == MVC_HOLD ? (N - 1) * nq : 0) + j];      // (a rest: no Bezier work)
                } else dev = cert_deviation(L.nodes + j, nq, nseg, cert_interval(n0, n_start, l, cur[c0 + sl]), &qm);
                L.dv[it] = dev;
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
            // B
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                const double *S = L.sk + 4 * s;
                const double D = cert_motion(L.rch + 7 * s, L.dv + sl * nq + 7 * L.sa[s]);
                double c[3];
                cert_centre(L.fr + (size_t)(sl * nq + L.sj[s]) * 12, S, c);
                L.cen[3 * it] = c[0]; L.cen[3 * it + 1] = c[1]; L.cen[3 * it + 2] = c[2];
                const double *TK = TL ? L.tk + (size_t)sl * n_tracks * 4 : nullptr;
                double dm = INFINITY, lm = INFINITY;
                int om = 0;
                for (int o = 0; o < n_obs; o++) {
                    const int k = TL ? L.tof[o] : -1;
                    double d, bound;
                    if (k >= 0) {
                        const double *M = TK + 4 * k;
                        d = clr_sd(L.ot[o], L.ok + 8 * o, c[0] - M[0], c[1] - M[1], c[2] - M[2]) - S[3];
                        bound = d - D - M[3];
                    } else {
                        d = clr_sd(L.ot[o], L.ok + 8 * o, c[0], c[1], c[2]) - S[3];
                        bound = d - D;
                    }
                    if (d < dm) { dm = d; om = o; }
                    if (TL) lm = fmin(lm, bound);
                }
                // Where the instantiations differ.  A track makes the smallest bound d - D_s - E_k a minimum of its own.  Without tracks it is the
                // bound of the smallest d, which the static certificate keeps: x -> fl(x - D_s) is monotone, and fmin drops a NaN where d < dm
                // does, so the two agree bit for bit (compared on the GPU, docs/HISTORY.md D.4)
                if (!TL) lm = dm - D;
                L.Dl[it] = D; L.pd[it] = dm; L.pl[it] = lm;
                const unsigned long long key = cert_key(cert_tkey(l, cur[c0 + sl]), s, 0, om);
                if (dm < INFINITY && cert_better(dm, key, B.d, B.k)) { B.d = dm; B.k = key; }
            }
            __syncthreads();
            // C
            if (pairs) {
                for (int it = tid; it < ns * nsph; it += CLR_NT) {
                    const int sl = it / nsph, s = it % nsph;
                    const double *C = L.cen + (size_t)sl * nsph * 3, *DD = L.Dl + (size_t)sl * nsph;
                    const double cx = C[3 * s], cy = C[3 * s + 1], cz = C[3 * s + 2], rs = L.sk[4 * s + 3], Dsv = DD[s];
                    const int as = L.sa[s], js = L.sj[s];
                    double dm = INFINITY, lm = INFINITY;
                    int tm = 0;
                    for (int t = s + 1; t < nsph; t++) {
                        if (!clr_pair(as, js, L.sa[t], L.sj[t], self_gap)) continue;      // (sj holds arm * 7 + joint: differences within one arm are joint differences)
                        const double ex = cx - C[3 * t], ey = cy - C[3 * t + 1], ez = cz - C[3 * t + 2];
                        const double d = sqrt(ex * ex + ey * ey + ez * ez) - rs - L.sk[4 * t + 3];
                        if (d < dm) { dm = d; tm = t; }
                        lm = fmin(lm, d - Dsv - DD[t]);
                    }
                    L.pd[it] = fmin(L.pd[it], dm); L.pl[it] = fmin(L.pl[it], lm);
                    const unsigned long long key = cert_key(cert_tkey(l, cur[c0 + sl]), s, 1, tm);
                    if (dm < INFINITY && cert_better(dm, key, B.d, B.k)) { B.d = dm; B.k = key; }
                }
                __syncthreads();
            }
            // D (chunk <= 16: the first wave decides; the other waves go on to the barrier that ends the chunk)
            if (tid < 64) {
                int what = -1, i = 0;
                double Lb = INFINITY;
                if (tid < ns) {
                    i = cur[c0 + tid];
                    double dmid = INFINITY;
                    for (int s = 0; s < nsph; s++) { dmid = fmin(dmid, L.pd[tid * nsph + s]); Lb = fmin(Lb, L.pl[tid * nsph + s]); }
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
    clr_reduce(B.d, B.k, nullptr);
    if (tid == 0) {
        mpcmp_clearance r;
        mpcmp_clearance_cert c;
        if (TL) cert_records(B, [&](unsigned tkey) { return mvc_time(tl, tkey); }, &r, &c);
        else {
            const double Te = p.d_sT[b];          // (read here, as the static certificate always did: it does not live in a register through the search)
            cert_records(B, [&](unsigned tkey) { return cert_time(n0, tkey) * Te; }, &r, &c);
        }
        out[b] = r;
        if (cert) cert[b] = c;
    }
}

// The two kernels: the one text above behind the argument lists their parents had.  The static certificate takes scalars, the timed one the
// shape, the tracks and the plans as structs: with one list for both, either kernel leaves the registers and the time it had as a kernel of its
// own (docs/HISTORY.md D.4)
__global__ __launch_bounds__(CLR_NT) void k_clearance_cert(const mpcmp_model *__restrict__ mdl, int narm, int nseg, const ClrSphere *__restrict__ sph,
                                                           int ns0, int ns1, const mpcmp_obstacle *__restrict__ obs, int n_obs, int obs_stride,
                                                           const double *__restrict__ sx, const double *__restrict__ sT, double margin, int self_gap,
                                                           int n_start, int max_depth, int chunk, mpcmp_clearance *__restrict__ out,
                                                           mpcmp_clearance_cert *__restrict__ cert) {
    const CertShape h = {narm, nseg, ns0, ns1, n_obs, obs_stride, chunk, n_start, 0, max_depth};
    const MvTracks none = {nullptr, nullptr, 0, 1, 0.0, 1.0};
    const CertPlans p = {sx, sT, nullptr, nullptr, nullptr};
    cert_search<false>(mdl, h, sph, obs, none, p, margin, self_gap, out, cert);
}
__global__ __launch_bounds__(CLR_NT) void k_clearance_cert_timed(const mpcmp_model *__restrict__ mdl, CertShape h, const ClrSphere *__restrict__ sph,
                                                                 const mpcmp_obstacle *__restrict__ obs, MvTracks trk, CertPlans p, double margin,
                                                                 int self_gap, mpcmp_clearance *__restrict__ out,
                                                                 mpcmp_clearance_cert *__restrict__ cert) {
    cert_search<true>(mdl, h, sph, obs, trk, p, margin, self_gap, out, cert);
}

hipError_t clearance_cert_prepare() {
    // the ceilings of both instantiations: two arms, 25 nodes, 256 obstacles and, with a timeline, 64 tracks
    for (int timed = 0; timed < 2; timed++) {
        const size_t mx = lds_ceiling([timed](int s) {
            return cert_lds_bytes(CertShape{2, 8, s, 0, CLR_MAX_OBS, 0, cert_chunk(s), 1, 1, 0}, timed != 0, timed ? MV_MAX_TRACKS : 0);
        });
        const hipError_t e = hipFuncSetAttribute(timed ? (const void *)k_clearance_cert_timed : (const void *)k_clearance_cert,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)mx);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t clearance_cert_launch(const ClrTables &t, const MvTracks *trk, const CertPlans &p, int B, double margin, int self_gap, int n_start,
                                 int n_rest, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st) {
    const int nsph = t.n_sph[0] + t.n_sph[1];
    const CertShape h = {t.narm, t.nseg, t.n_sph[0], t.n_sph[1], t.n_obs, t.obs_stride, cert_chunk(nsph), n_start, n_rest, max_depth};
    const size_t lds = cert_lds_bytes(h, trk != nullptr, trk ? trk->n_tracks : 0);
    if (trk) hipLaunchKernelGGL(k_clearance_cert_timed, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, t.d_sph, t.d_obs, *trk, p, margin, self_gap, d_out, d_cert);
    else hipLaunchKernelGGL(k_clearance_cert, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h.narm, h.nseg, t.d_sph, h.ns0, h.ns1, t.d_obs, h.n_obs, h.obs_stride,
                            p.d_sx, p.d_sT, margin, self_gap, h.n_start, h.max_depth, h.chunk, d_out, d_cert);
    return hipGetLastError();
}

}  // namespace mpcmp
