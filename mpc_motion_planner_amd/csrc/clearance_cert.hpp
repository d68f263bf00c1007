// clearance_cert.hpp — the rule of the certified clearance check (include/mpcmp_clearance_cert.h) as host/device functions: the geometry of an
// interval, the Bezier deviation of a joint, the reach table, the frames of one arm, the decision, the tie keys, the two records and the kernel's LDS
// layout.  The kernel (clearance_cert.hip, with and without a timeline) and the host statements of model_host.cpp both run this source.  Plain C++: no HIP header, and nothing here is a kernel.
#pragma once
#include <cmath>
#include <cstddef>
#include "clearance_rule.hpp"
#include "plan_interp.hpp"

namespace mpcmp {

constexpr int CERT_CAP = MPCMP_CLR_CERT_CAPACITY;   // intervals per level
constexpr int CERT_SPLIT = CERT_CAP / 2;            // intervals of one level that may be split
constexpr int CERT_MAX_DEPTH = 16;

// Interval (l, i) of n0 = nseg n_start level-0 intervals: its segment, its ends and midpoint in normalised time, its width.  Every quotient has an
// exact numerator and an exact denominator (below 2^30), so a time is the correctly rounded value of its fraction however it is reached.
struct CertInterval {
    int seg;
    double ta, tm, tb, h;
};
MPCMP_HD CertInterval cert_interval(int n0, int n_start, int l, int i) {
    CertInterval v;
    const double den = (double)n0 * (double)(1 << l);
    v.seg = (i >> l) / n_start;
    v.ta = (double)i / den;
    v.tb = (double)(i + 1) / den;
    v.tm = (double)(2 * i + 1) / (2.0 * den);
    v.h = 1.0 / den;
    return v;
}

// The order of midpoints across levels as an integer: t_m = key / (n0 2^17), key = (2 i + 1) 2^(16 - l) < 2^29; distinct intervals have distinct keys
MPCMP_HD unsigned cert_tkey(int l, int i) { return (unsigned)(2 * i + 1) << (CERT_MAX_DEPTH - l); }
MPCMP_HD double cert_time(int n0, unsigned tkey) { return (double)tkey / ((double)n0 * 131072.0); }
constexpr unsigned CERT_NO_TIME = 0xFFFFFFFFu;

// Ties of d_min: lowest midpoint, then lowest sphere, then obstacles before robot pairs, then lowest index = the order of this key (clr_pack with the
// midpoint key in place of the sample).  Ties of d_lower: lowest midpoint = the same key with the low 16 bits 0
MPCMP_HD unsigned long long cert_key(unsigned tkey, int sphere, int robot, int idx) {
    return ((unsigned long long)tkey << 16) | ((unsigned long long)sphere << 9) | ((unsigned long long)robot << 8) | (unsigned long long)idx;
}
constexpr unsigned long long CERT_NO_PAIR = ~0ull;
MPCMP_HD bool cert_better(double d, unsigned long long k, double bd, unsigned long long bk) { return clr_better(d, k, bd, bk); }

// dev of one joint column on an interval, and q(t_m): C points at the column in node 0, `stride` doubles lie between two nodes
MPCMP_HD double cert_deviation(const double *C, int stride, int nseg, const CertInterval &v, double *q_m) {
    double W[4];
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.tm, W);
    const double qm = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.ta, W);
    const double b0 = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_derivative_on_segment(nseg, v.seg, v.ta, W);
    const double b1 = b0 + (v.h / 3.0) * mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.tb, W);
    const double b3 = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_derivative_on_segment(nseg, v.seg, v.tb, W);
    const double b2 = b3 - (v.h / 3.0) * mpcmp_plan::interp_channel(C, stride, v.seg, W);
    *q_m = qm;
    return fmax(fmax(fabs(b0 - qm), fabs(b1 - qm)), fmax(fabs(b2 - qm), fabs(b3 - qm)));
}

// reach [7] of a sphere with the centre c on joint `joint` of the arm whose joint offsets are p(k) = P[pstride k .. + 3]: entries above `joint` are 0,
// so that D_s is one sum over the arm's seven deviations
MPCMP_HD void cert_reach(const double *P, int pstride, int joint, const double *c, double *reach) {
    double r = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int i = 6; i > joint; i--) reach[i] = 0.0;
    for (int i = joint; i >= 0; i--) {
        reach[i] = r;
        const double *p = P + pstride * i;
        r += sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    }
}
MPCMP_HD double cert_motion(const double *reach, const double *dev) {
    double D = 0.0;
    for (int i = 0; i < 7; i++) D += reach[i] * dev[i];
    return D;
}

// World rotation and origin of the seven joint frames of one arm, F [7][12] = Rw (9), pw (3), from its placements M [7][12] = R0 (9), p (3) and the
// sines and cosines SC [7][2] of its joints: p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i)
MPCMP_HD void cert_frames(const double *M, const double *SC, double *F) {
    double Rw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pw[3] = {0, 0, 0};
    PLAN_UNROLL
    for (int i = 0; i < 7; i++) {
        const double *A = M + 12 * i;
        const double s = SC[2 * i], c = SC[2 * i + 1];
        double R[9], Rn[9];
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) {
            R[3 * r] = A[3 * r] * c + A[3 * r + 1] * s;
            R[3 * r + 1] = -A[3 * r] * s + A[3 * r + 1] * c;
            R[3 * r + 2] = A[3 * r + 2];
        }
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) pw[r] += Rw[3 * r] * A[9] + Rw[3 * r + 1] * A[10] + Rw[3 * r + 2] * A[11];
        PLAN_UNROLL
        for (int r = 0; r < 3; r++)
            PLAN_UNROLL
            for (int c2 = 0; c2 < 3; c2++) Rn[3 * r + c2] = Rw[3 * r] * R[c2] + Rw[3 * r + 1] * R[3 + c2] + Rw[3 * r + 2] * R[6 + c2];
        PLAN_UNROLL
        for (int k = 0; k < 9; k++) { Rw[k] = Rn[k]; F[12 * i + k] = Rn[k]; }
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) F[12 * i + 9 + r] = pw[r];
    }
}
// world centre of a sphere with the centre c in the frame F [12] of its joint
MPCMP_HD void cert_centre(const double *F, const double *c, double *w) {
    w[0] = F[9] + F[0] * c[0] + F[1] * c[1] + F[2] * c[2];
    w[1] = F[10] + F[3] * c[0] + F[4] * c[1] + F[5] * c[2];
    w[2] = F[11] + F[6] * c[0] + F[7] * c[1] + F[8] * c[2];
}

// the decision of one interval (the order is part of the rule; a NaN never certifies: it ends as UNDECIDED or is split)
enum { CERT_HIT = 0, CERT_CLEAR = 1, CERT_UNDECIDED = 2, CERT_SPLIT_IT = 3 };
MPCMP_HD int cert_decide(double d_mid, double L, double margin, int l, int max_depth) {
    if (d_mid < margin) return CERT_HIT;
    if (L >= margin) return CERT_CLEAR;
    if (l == max_depth) return CERT_UNDECIDED;
    return CERT_SPLIT_IT;
}

// What the search keeps: the best (d, key) over every pair met, the best (L, key) and the counts over the leaves, the earliest hit, the last level
struct CertBest {
    double d = INFINITY, L = INFINITY;
    unsigned long long k = CERT_NO_PAIR, Lk = CERT_NO_PAIR;
    unsigned first = CERT_NO_TIME;
    int n_hit = 0, n_clear = 0, n_und = 0, n_eval = 0, depth = 0;
};
// ... and the two records made of it; time_of turns a midpoint key into a record time (cert_time x T, or mvc_time of moving_cert_rule.hpp)
template <class TimeOf> MPCMP_HD void cert_records(const CertBest &s, TimeOf time_of, mpcmp_clearance *r, mpcmp_clearance_cert *c) {
    r->d_min = s.d;
    if (s.k == CERT_NO_PAIR) { r->t_min = -1.0; r->sphere = -1; r->other = 0; }
    else {
        r->t_min = time_of((unsigned)(s.k >> 16));
        clr_unpack(s.k, &r->sphere, &r->other);
    }
    r->t_first = s.first != CERT_NO_TIME ? time_of(s.first) : -1.0;
    r->n_hit = s.n_hit;
    r->status = (s.n_hit > 0 ? MPCMP_CLR_HIT : 0) | (s.n_und > 0 ? MPCMP_CLR_UNDECIDED : 0);
    c->d_lower = s.L; c->t_lower = time_of((unsigned)(s.Lk >> 16));
    c->n_eval = s.n_eval; c->n_clear = s.n_clear; c->n_undecided = s.n_und; c->depth = s.depth;
}
// the certificate that goes with clr_nan_record()
MPCMP_HD mpcmp_clearance_cert cert_nan_record() {
    mpcmp_clearance_cert c;
    c.d_lower = NAN; c.t_lower = -1.0; c.n_eval = 0; c.n_clear = 0; c.n_undecided = 0; c.depth = 0;
    return c;
}

// intervals per chunk: as many as keep chunk x spheres <= 512 per-sphere records in LDS, at most 16 (one lane of the first wave decides each)
inline int cert_chunk(int nsph) {
    const int c = nsph > 0 ? 512 / nsph : 16;
    return c > 16 ? 16 : (c < 1 ? 1 : c);
}
// The dynamic LDS of k_clearance_cert: the tables, the chunk and the two level lists; with a timeline also the chunk's track table (n_tracks tracks)
// and the obstacles' tracks, which the static certificate does not pay for.  It does not depend on n_start, n_rest or max_depth
struct CertShape { int narm, nseg, ns0, ns1, n_obs, obs_stride, chunk, n_start, n_rest, max_depth; };
struct CertLds {
    double *mk, *nodes, *sk, *rch, *ok, *sc, *dv, *fr, *cen, *Dl, *pd, *pl, *tk;
    int *cur, *nxt, *sj, *sa, *ot, *tof, *end;
};
// The layout: plain pointer arithmetic on the LDS base, stated once as the text below.  The kernel expands it among its own locals; cert_layout
// expands it for the launch's byte count and for tests/host/clearance_lds_check.cpp.  It is neither a carve over the cursor of clearance_lds.hpp, as
// the sampled kernels have it, nor a function the kernel calls: through either the kernel with a timeline compiles to other code and is 0.5 - 0.9 %
// slower (docs/HISTORY.md D.4).  TL_: with a timeline; L.end: where the last array ends
#define MPCMP_CERT_LAYOUT(L, lds, narm, nq, N, nsph, n_obs, chunk, TL_, n_tracks)                                                                    \
    L.mk = lds;                                              /* [narm][7][12] = R0 (9), p (3) */                                                      \
    L.nodes = L.mk + 84 * narm;                              /* [N][nq] */                                                                            \
    L.sk = L.nodes + (size_t)nq * N;                         /* [nsph][4] = c, r */                                                                   \
    L.rch = L.sk + 4 * nsph;                                 /* [nsph][7] */                                                                          \
    L.ok = L.rch + 7 * nsph;                                 /* [n_obs][8] */                                                                         \
    L.sc = L.ok + 8 * n_obs;                                 /* [chunk][nq][2] */                                                                     \
    L.dv = L.sc + (size_t)chunk * nq * 2;                    /* [chunk][nq] */                                                                        \
    L.fr = L.dv + (size_t)chunk * nq;                        /* [chunk][nq][12] = Rw (9), pw (3) */                                                   \
    L.cen = L.fr + (size_t)chunk * nq * 12;                  /* [chunk][nsph][3] */                                                                   \
    L.Dl = L.cen + (size_t)chunk * nsph * 3;                 /* [chunk][nsph] D_s */                                                                  \
    L.pd = L.Dl + (size_t)chunk * nsph;                      /* [chunk][nsph] smallest d of the sphere's pairs */                                     \
    L.pl = L.pd + (size_t)chunk * nsph;                      /* [chunk][nsph] smallest bound of the sphere's pairs */                                 \
    L.tk = L.pl + (size_t)chunk * nsph;                      /* [chunk][n_tracks][4] = p_m (3), E_k (with a timeline) */                              \
    L.cur = reinterpret_cast<int *>(L.tk + (TL_ ? (size_t)chunk * n_tracks * 4 : 0));      /* [CERT_CAP] */                                           \
    L.nxt = L.cur + CERT_CAP;                                /* [CERT_CAP] */                                                                         \
    L.sj = L.nxt + CERT_CAP;                                 /* [nsph] arm * 7 + joint */                                                             \
    L.sa = L.sj + nsph;                                      /* [nsph] arm */                                                                         \
    L.ot = L.sa + nsph;                                      /* [n_obs] type */                                                                       \
    L.tof = L.ot + n_obs;                                    /* [n_obs] track, -1: none (with a timeline) */                                          \
    L.end = L.tof + (TL_ ? n_obs : 0);
inline CertLds cert_layout(double *lds, const CertShape &h, bool timeline, int n_tracks) {
    const int narm = h.narm, N = 3 * h.nseg + 1, nq = 7 * narm, nsph = h.ns0 + h.ns1, n_obs = h.n_obs, chunk = h.chunk;
    CertLds L;
    MPCMP_CERT_LAYOUT(L, lds, narm, nq, N, nsph, n_obs, chunk, timeline, n_tracks)
    return L;
}
// the bytes of that layout, a whole number of doubles: the layout itself on a base that is never read (one double, so that no pointer is null)
inline size_t cert_lds_bytes(const CertShape &h, bool timeline, int n_tracks) {
    static double base[1];
    const CertLds L = cert_layout(base, h, timeline, n_tracks);
    return ((size_t)(reinterpret_cast<const char *>(L.end) - reinterpret_cast<const char *>(base)) + 7) / 8 * 8;
}

}  // namespace mpcmp
