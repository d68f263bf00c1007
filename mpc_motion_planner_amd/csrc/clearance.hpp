// clearance.hpp — what the clearance checker shares between the host entry points (mpcmp.hip), its kernels (clearance.hip) and the host
// restatement mpcmp_clearance_config: the obstacle distance formulas, the pair rules, the ordering of ties, the LDS budget and the launchers.
// The kernels themselves live in clearance.hip, a translation unit of their own: nothing here is a kernel, so including this header does not
// change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "../../include/mpcmp.h"

namespace mpcmp {

constexpr int CLR_MAX_SPH = 64;      // robot spheres per arm
constexpr int CLR_MAX_OBS = 256;     // obstacles per set
constexpr int CLR_MAX_PTS = 4096;    // n_pts
constexpr int CLR_NT = 256;          // threads per workgroup of k_clearance

// a robot sphere as the kernel reads it (mpcmp_sphere plus its arm); table order = arm-major = the numbering of mpcmp_clearance.sphere
struct ClrSphere {
    double c[3], r;
    int joint, arm;
};

// An obstacle in the form the distance function reads, k[8] = a(3), b'(3), r, w: for a capsule b' = b - a and w = 1 / |b - a|^2 (0 when a == b),
// formed once per obstacle instead of once per pair; every other type b' = b, w = 0.
__host__ __device__ inline void clr_obs_prepare(const mpcmp_obstacle &o, double *k) {
    for (int d = 0; d < 3; d++) { k[d] = o.a[d]; k[3 + d] = o.b[d]; }
    k[6] = o.r; k[7] = 0.0;
    if (o.type == MPCMP_OBS_CAPSULE) {
        double l2 = 0.0;
        for (int d = 0; d < 3; d++) { k[3 + d] = o.b[d] - o.a[d]; l2 += k[3 + d] * k[3 + d]; }
        k[7] = l2 > 0.0 ? 1.0 / l2 : 0.0;
    }
}

// signed distance of the world point (x, y, z) to an obstacle (include/mpcmp.h, "Signed distance")
__host__ __device__ inline double clr_sd(int type, const double *k, double x, double y, double z) {
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
__host__ __device__ inline bool clr_pair(int arm_s, int joint_s, int arm_t, int joint_t, int self_gap) {
    if (arm_s != arm_t) return true;
    const int d = joint_s > joint_t ? joint_s - joint_t : joint_t - joint_s;
    return self_gap > 0 && d >= self_gap;
}

// Ties of d_min: lowest sample, then lowest sphere, then obstacles before robot pairs, then lowest index = the order of this key.
// sample < 2^13, sphere < 2^7, index < 2^8.
__host__ __device__ inline unsigned clr_pack(int ip, int sphere, int robot, int idx) {
    return ((unsigned)ip << 17) | ((unsigned)sphere << 9) | ((unsigned)robot << 8) | (unsigned)idx;
}
constexpr unsigned CLR_NO_PAIR = 0xFFFFFFFFu;
__host__ __device__ inline bool clr_better(double d, unsigned k, double bd, unsigned bk) { return d < bd || (d == bd && k < bk); }

// a double as an unsigned key of the same order (the key of time_sync.hpp, restated here because that header defines kernels)
__host__ __device__ inline unsigned long long clr_tkey(double x) {
    unsigned long long u;
    __builtin_memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// samples per chunk: as many as keep chunk x spheres <= 1024 world centres in LDS, at most 32
inline int clr_chunk(int nsph) {
    const int c = nsph > 0 ? 1024 / nsph : 32;
    return c > 32 ? 32 : (c < 1 ? 1 : c);
}
// dynamic LDS of k_clearance in bytes: it depends on the tables and the chunk, not on n_pts
inline size_t clr_lds_bytes(int narm, int N, int nsph, int n_obs, int chunk) {
    const size_t dbl = (size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 14 +
                       (size_t)chunk * narm * 84 + (size_t)chunk * nsph * 3;
    const size_t ints = (size_t)2 * nsph + (size_t)n_obs + (size_t)chunk;
    return dbl * sizeof(double) + (ints + 1) / 2 * 2 * sizeof(int);
}

struct ClrTables {
    const mpcmp_model *d_model;      // [narm]
    int narm, nseg;
    const ClrSphere *d_sph;          // [n_sph[0] + n_sph[1]]
    int n_sph[2];
    const mpcmp_obstacle *d_obs;     // [n_sets][n_obs]
    int n_obs, obs_stride;           // obs_stride: 0 (one world) or n_obs (set b for problem b)
};

hipError_t clearance_prepare();     // the kernel's dynamic-LDS ceiling; called by a context's first check
hipError_t clearance_launch(const ClrTables &t, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                            mpcmp_clearance *d_out, hipStream_t st);
// keys [n_groups] scratch; chosen [n_groups].  d_clr and d_lim may each be NULL (that test is skipped); lim_mask: the bits of mpcmp_limits.status that
// make a member inadmissible (MPCMP_LIM_NAN always does)
hipError_t select_launch(int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr, const mpcmp_limits *d_lim, int lim_mask,
                         const int *d_group, int n_groups, unsigned long long *d_keys, int *d_chosen, hipStream_t st);

}  // namespace mpcmp
