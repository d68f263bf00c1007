// clearance_lds.hpp — the dynamic LDS of the clearance kernels.  A layout is ONE host/device function, a carve, that hands its arrays out of a
// cursor in order: the kernel carves its LDS with it, and the launch asks for the bytes the same function counts on a cursor without a base, so a
// size and a layout cannot disagree.  Here: the cursor, the chunk rule and the carve of the sampled kernels (k_clearance, the three of moving.hip,
// k_clearance_field); the certified kernel's layout, plain pointer arithmetic stated once, is in clearance_cert.hpp.  Plain C++: tests/host/clearance_lds_check.cpp reads it without HIP.
#pragma once
#include <cstddef>
#include "clearance_rule.hpp"

namespace mpcmp {

// REAL: each array starts where the one before it ends, from `at` on; otherwise null pointers, and only the bytes are counted.  Every carve takes
// its 8-byte arrays first and its ints last
template <bool REAL> struct LdsCursor {
    char *at;
    size_t bytes;
    // (the count keeps its type: an int count is added to the pointer as an int, as in hand-written layout code, which the kernels compile from best)
    template <class T, class N> MPCMP_HD T *take(N n) {
        T *p = REAL ? reinterpret_cast<T *>(at) : nullptr;
        if (REAL) at = reinterpret_cast<char *>(p + n);
        else bytes += (size_t)n * sizeof(T);
        return p;
    }
};
// the bytes of a layout, a whole number of doubles: carve is called with a cursor and nothing else
template <class F> inline size_t lds_bytes(F carve) {
    LdsCursor<false> c = {nullptr, 0};
    carve(c);
    return (c.bytes + 7) / 8 * 8;
}
// the ceiling of a layout over every sphere count (the chunk shrinks as the sphere tables grow): what a kernel is allowed before its first launch
template <class F> inline size_t lds_ceiling(F bytes_of_nsph) {
    size_t mx = 0;
    for (int s = 0; s <= 2 * CLR_MAX_SPH; s++) {
        const size_t b = bytes_of_nsph(s);
        if (b > mx) mx = b;
    }
    return mx;
}

// samples per chunk: as many as keep chunk x spheres <= 1024 world centres in LDS, at most 32
inline int clr_chunk(int nsph) {
    const int c = nsph > 0 ? 1024 / nsph : 32;
    return c > 32 ? 32 : (c < 1 ? 1 : c);
}

// what a sampled kernel is launched for: arms, segments, spheres per arm, obstacles per set, doubles between two sets (0: one world), the chunk
struct ClrShape { int narm, nseg, n0, n1, n_obs, obs_stride, chunk; };
// the three layouts: k_clearance; the kernels of a moving world (the clock of a chunk's samples, the tracks' indices and, for k_start_delay, K
// delays); k_clearance_field (no obstacle, no pair: neither centres nor arms)
enum { CLR_LDS_SAMPLED = 0, CLR_LDS_TIMED = 1, CLR_LDS_FIELD = 2 };
struct ClrLds {
    double *mk, *nodes, *sk, *ok, *sc, *fr, *cen, *ss, *tt, *pf, *dly;
    unsigned long long *dk, *w0;
    int *sj, *sa, *ot, *tof, *lst, *hit, *pk, *pk1;
};
template <bool REAL> MPCMP_HD ClrLds clr_carve(LdsCursor<REAL> &c, const ClrShape &h, int kind, int K) {
    const size_t N = 3 * h.nseg + 1, nq = 7 * h.narm, nsph = h.n0 + h.n1, nobs = h.n_obs, ch = h.chunk;
    const size_t tm = kind == CLR_LDS_TIMED ? 1 : 0, pr = kind == CLR_LDS_FIELD ? 0 : 1;
    ClrLds L;
    L.mk = c.template take<double>(84 * h.narm);             // [narm][7][12] = R0 (9), p (3)
    L.nodes = c.template take<double>(nq * N);               // [N][nq]
    L.sk = c.template take<double>(4 * nsph);                // [nsph][4] = c, r
    L.ok = c.template take<double>(8 * nobs);                // [n_obs][8]
    L.sc = c.template take<double>(ch * nq * 2);             // [chunk][nq][2]
    L.fr = c.template take<double>(ch * nq * 12);            // [chunk][nq][12] = Rw (9), pw (3)
    L.cen = c.template take<double>(pr * ch * nsph * 3);     // [chunk][nsph][3]
    L.ss = c.template take<double>(tm * ch);                 // [chunk] normalised plan time
    L.tt = c.template take<double>(tm * ch);                 // [chunk] running time
    L.pf = c.template take<double>(tm * ch);                 // [chunk] weight of the later key
    L.dly = c.template take<double>(tm * K);                 // [K]
    L.dk = c.template take<unsigned long long>(tm * K);      // [K] ordered keys of the runs' minima over the tracked obstacles
    L.w0 = c.template take<unsigned long long>(tm * K);      // [K] ... of the start posture at the world times delays[k]
    L.sj = c.template take<int>(nsph);                       // [nsph] arm * 7 + joint
    L.sa = c.template take<int>(pr * nsph);                  // [nsph] arm
    L.ot = c.template take<int>(nobs);                       // [n_obs] type
    L.tof = c.template take<int>(tm * nobs);                 // [n_obs] track, -1: none
    L.lst = c.template take<int>(tm * nobs);                 // [n_obs] the tracked obstacles first, then the others (k_start_delay)
    L.hit = c.template take<int>(ch);                        // [chunk]
    L.pk = c.template take<int>(tm * ch);                    // [chunk] earlier key
    L.pk1 = c.template take<int>(tm * ch);                   // [chunk] later key
    if (!pr) L.sa = nullptr;                                 // (staging skips it)
    return L;
}
inline size_t clr_lds_bytes(const ClrShape &h, int kind, int K) {
    return lds_bytes([&](LdsCursor<false> &c) { clr_carve(c, h, kind, K); });
}

}  // namespace mpcmp
