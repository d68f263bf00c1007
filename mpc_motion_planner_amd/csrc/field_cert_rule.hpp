// field_cert_rule.hpp — what the certified clearance check against a voxel world (include/mpcmp_field_cert.h) adds to the rules it is made of:
// the distance of one sphere at an interval's midpoint, the tie key of d_min, the merge of two certificates, and the chunk and the LDS layout of
// k_clearance_cert_field.  Everything else is clearance_cert.hpp (intervals, deviations, reach, frames, the decision, the records) and
// field_rule.hpp (fld_sd), called and not restated.  Plain C++: the kernel (field_cert.hip), the host statement (model_host.cpp) and
// tests/host/field_cert_lds_check.cpp read this one source.  Nothing here is a kernel.
#pragma once
#include <cmath>
#include <cstddef>
#include "clearance_cert.hpp"
#include "field_rule.hpp"

namespace mpcmp {

// d_s of a sphere with the world centre c [3] and the radius r at a midpoint, and the voxel read.  The bound of its interval is d_s - D_s
// (cert_motion): sd_field lies below the true distance, which is 1-Lipschitz, so the true clearance on the interval is at least that
MPCMP_HD double fcert_distance(const mpcmp_field_desc &g, const unsigned *d2, const double *c, double r, int *voxel) {
    return fld_sd(g, d2, c[0], c[1], c[2], voxel) - r;
}

// Ties of d_min: lowest midpoint, then lowest sphere = cert_key without a partner.  The voxel follows from the two, so it is carried beside the key
// and is no part of it; cert_records leaves `other` 0 and the caller writes the voxel over it
MPCMP_HD unsigned long long fcert_key(unsigned tkey, int sphere) { return cert_key(tkey, sphere, 0, 0); }

// two certificates of one plan as one (include/mpcmp_field_cert.h, mpcmp_clearance_cert_merge_batch)
MPCMP_HD mpcmp_clearance_cert fcert_merge(const mpcmp_clearance_cert &a, const mpcmp_clearance_cert &b) {
    if (a.d_lower != a.d_lower || b.d_lower != b.d_lower) return cert_nan_record();
    mpcmp_clearance_cert o;
    const bool second = b.d_lower < a.d_lower;           // (ties stay with a)
    o.d_lower = second ? b.d_lower : a.d_lower;
    o.t_lower = second ? b.t_lower : a.t_lower;
    o.n_eval = a.n_eval + b.n_eval; o.n_clear = a.n_clear + b.n_clear; o.n_undecided = a.n_undecided + b.n_undecided;
    o.depth = a.depth > b.depth ? a.depth : b.depth;
    return o;
}

// Intervals per chunk of k_clearance_cert_field: as many as keep the chunk's arrays (15 doubles per joint and 2 per sphere for each interval) within
// FCERT_CHUNK_DOUBLES, at most FCERT_CHUNK_MAX (one lane of the first wave decides each, so 64 is the ceiling of the structure).  The rule does not
// depend on the chunk; both constants are chosen by measurement ("Certified clearance against voxel worlds")
constexpr int FCERT_CHUNK_MAX = 32;
constexpr int FCERT_CHUNK_DOUBLES = 5120;
inline int fcert_chunk(int narm, int nsph) {
    const int c = FCERT_CHUNK_DOUBLES / (105 * narm + 2 * nsph);
    return c > FCERT_CHUNK_MAX ? FCERT_CHUNK_MAX : (c < 1 ? 1 : c);
}
// the pitch of the per-sphere rows pd and pl: odd, so that the lanes of phase B (neighbouring spheres of one interval) write to different banks
// while the deciding lanes of phase D (neighbouring intervals of one sphere) read neighbouring doubles
MPCMP_HD int fcert_pitch(int chunk) { return chunk | 1; }

// The dynamic LDS of k_clearance_cert_field: the tables, the chunk and the two level lists.  No obstacle, no world centre and no D_s is kept: a
// sphere's distance and bound are final in phase B.  It does not depend on n_start or max_depth
struct FcertShape { int narm, nseg, ns0, ns1, chunk, n_start, max_depth; };
struct FcertLds {
    double *mk, *nodes, *sk, *rch, *sc, *dv, *fr, *pd, *pl;
    int *cur, *nxt, *sj, *sa, *end;
};
// the layout, stated once as MPCMP_CERT_LAYOUT is: the kernel expands it among its own locals, fcert_layout for the launch's byte count and for the
// host check.  L.end: where the last array ends
#define MPCMP_FCERT_LAYOUT(L, lds, narm, nq, N, nsph, chunk)                                                                                         \
    L.mk = lds;                                              /* [narm][7][12] = R0 (9), p (3) */                                                      \
    L.nodes = L.mk + 84 * narm;                              /* [N][nq] */                                                                            \
    L.sk = L.nodes + (size_t)nq * N;                         /* [nsph][4] = c, r */                                                                   \
    L.rch = L.sk + 4 * nsph;                                 /* [nsph][7] */                                                                          \
    L.sc = L.rch + 7 * nsph;                                 /* [chunk][nq][2] */                                                                     \
    L.dv = L.sc + (size_t)chunk * nq * 2;                    /* [chunk][nq] */                                                                        \
    L.fr = L.dv + (size_t)chunk * nq;                        /* [chunk][nq][12] = Rw (9), pw (3) */                                                   \
    L.pd = L.fr + (size_t)chunk * nq * 12;                   /* [nsph][pitch] d_s */                                                                  \
    L.pl = L.pd + (size_t)nsph * fcert_pitch(chunk);         /* [nsph][pitch] d_s - D_s */                                                            \
    L.cur = reinterpret_cast<int *>(L.pl + (size_t)nsph * fcert_pitch(chunk));             /* [CERT_CAP] */                                           \
    L.nxt = L.cur + CERT_CAP;                                /* [CERT_CAP] */                                                                         \
    L.sj = L.nxt + CERT_CAP;                                 /* [nsph] arm * 7 + joint */                                                             \
    L.sa = L.sj + nsph;                                      /* [nsph] arm */                                                                         \
    L.end = L.sa + nsph;
inline FcertLds fcert_layout(double *lds, const FcertShape &h) {
    const int narm = h.narm, N = 3 * h.nseg + 1, nq = 7 * narm, nsph = h.ns0 + h.ns1, chunk = h.chunk;
    FcertLds L;
    MPCMP_FCERT_LAYOUT(L, lds, narm, nq, N, nsph, chunk)
    return L;
}
// the bytes of that layout, a whole number of doubles (the layout on a base that is never read)
inline size_t fcert_lds_bytes(const FcertShape &h) {
    static double base[1];
    const FcertLds L = fcert_layout(base, h);
    return ((size_t)(reinterpret_cast<const char *>(L.end) - reinterpret_cast<const char *>(base)) + 7) / 8 * 8;
}

}  // namespace mpcmp
