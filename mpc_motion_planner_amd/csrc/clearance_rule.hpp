// clearance_rule.hpp — the part of the clearance rule that is plain arithmetic: the obstacle distance formulas, the pair rule and the ordering of
// ties (include/mpcmp.h, "clearance").  Plain C++, so that the host-only unit (model_host.cpp) reads the same source as the kernels; clearance.hpp
// includes it.  Nothing here is a kernel.
#pragma once
#include <cmath>
#include "../../include/mpcmp.h"

// (the macro of kinematics_host.hpp, token for token, so that either file may come first)
#ifndef MPCMP_HD
#ifdef __HIPCC__
#define MPCMP_HD __host__ __device__ inline
#else
#define MPCMP_HD inline
#endif
#endif

namespace mpcmp {

constexpr int CLR_MAX_SPH = 64;      // robot spheres per arm
constexpr int CLR_MAX_OBS = 256;     // obstacles per set

// An obstacle in the form the distance function reads, k[8] = a(3), b'(3), r, w: for a capsule b' = b - a and w = 1 / |b - a|^2 (0 when a == b),
// formed once per obstacle instead of once per pair; every other type b' = b, w = 0.
MPCMP_HD void clr_obs_prepare(const mpcmp_obstacle &o, double *k) {
    for (int d = 0; d < 3; d++) { k[d] = o.a[d]; k[3 + d] = o.b[d]; }
    k[6] = o.r; k[7] = 0.0;
    if (o.type == MPCMP_OBS_CAPSULE) {
        double l2 = 0.0;
        for (int d = 0; d < 3; d++) { k[3 + d] = o.b[d] - o.a[d]; l2 += k[3 + d] * k[3 + d]; }
        k[7] = l2 > 0.0 ? 1.0 / l2 : 0.0;
    }
}

// signed distance of the world point (x, y, z) to an obstacle (include/mpcmp.h, "Signed distance")
MPCMP_HD double clr_sd(int type, const double *k, double x, double y, double z) {
    const double dx = x - k[0], dy = y - k[1], dz = z - k[2];
    if (type == MPCMP_OBS_SPHERE) return sqrt(dx * dx + dy * dy + dz * dz) - k[6];
    if (type == MPCMP_OBS_CAPSULE) {
        double t = (dx * k[3] + dy * k[4] + dz * k[5]) * k[7];
        t = fmin(fmax(t, 0.0), 1.0);
        const double ex = dx - t * k[3], ey = dy - t * k[4], ez = dz - t * k[5];
        return sqrt(ex * ex + ey * ey + ez * ez) - k[6];
    }
    if (type == MPCMP_OBS_BOX) {
        const double qx = fabs(dx) - k[3], qy = fabs(dy) - k[4], qz = fabs(dz) - k[5];
        const double ox = fmax(qx, 0.0), oy = fmax(qy, 0.0), oz = fmax(qz, 0.0);
        return sqrt(ox * ox + oy * oy + oz * oz) + fmin(fmax(qx, fmax(qy, qz)), 0.0) - k[6];
    }
    return k[0] * x + k[1] * y + k[2] * z - k[3];      // MPCMP_OBS_HALFSPACE
}

// robot pair (s, t), s < t in table order: always across arms; within one arm only with self_gap > 0 and joint indices at least self_gap apart
MPCMP_HD bool clr_pair(int arm_s, int joint_s, int arm_t, int joint_t, int self_gap) {
    if (arm_s != arm_t) return true;
    const int d = joint_s > joint_t ? joint_s - joint_t : joint_t - joint_s;
    return self_gap > 0 && d >= self_gap;
}

// Ties of d_min: lowest sample, then lowest sphere, then obstacles before robot pairs, then lowest index = the order of this key.
// sample < 2^13, sphere < 2^7, index < 2^8.
MPCMP_HD unsigned clr_pack(int ip, int sphere, int robot, int idx) {
    return ((unsigned)ip << 17) | ((unsigned)sphere << 9) | ((unsigned)robot << 8) | (unsigned)idx;
}
constexpr unsigned CLR_NO_PAIR = 0xFFFFFFFFu;
template <class K> MPCMP_HD bool clr_better(double d, K k, double bd, K bk) { return d < bd || (d == bd && k < bk); }

// The low 16 bits of a key, which clr_pack and cert_key (clearance_cert.hpp) share: the sphere, and the obstacle's index or -1 - the partner sphere
MPCMP_HD void clr_unpack(unsigned long long k, int *sphere, int *other) {
    const int idx = (int)(k & 0xFFu);
    *sphere = (int)((k >> 9) & 0x7Fu);
    *other = (k & 0x100u) ? -1 - idx : idx;
}
// the MPCMP_CLR_NAN record, the one statement of it for every member of the family on the host and on the device
MPCMP_HD mpcmp_clearance clr_nan_record() {
    mpcmp_clearance r;
    r.d_min = NAN; r.t_min = -1.0; r.t_first = -1.0; r.sphere = -1; r.other = 0; r.n_hit = 0; r.status = MPCMP_CLR_NAN;
    return r;
}
// the record of a sampled check from its best (d, key), the first sample that hit and the count of those: sample ip lies at (ip / n_pts) T_run
MPCMP_HD mpcmp_clearance clr_record(double best_d, unsigned best_k, int first, int n_hit, int n_pts, double T_run) {
    mpcmp_clearance r;
    r.d_min = best_d;
    if (best_k == CLR_NO_PAIR) { r.t_min = -1.0; r.sphere = -1; r.other = 0; }
    else {
        r.t_min = ((double)(int)(best_k >> 17) / n_pts) * T_run;
        clr_unpack(best_k, &r.sphere, &r.other);
    }
    r.t_first = first >= 0 ? ((double)first / n_pts) * T_run : -1.0;
    r.n_hit = n_hit;
    r.status = n_hit > 0 ? MPCMP_CLR_HIT : 0;
    return r;
}

// a double as an unsigned key of the same order (the key of time_sync.hpp, restated here because that header defines kernels)
MPCMP_HD unsigned long long clr_tkey(double x) {
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

}  // namespace mpcmp
