// clearance.hpp — what the clearance checker shares between the host entry points (mpcmp.hip), its kernels (clearance.hip) and the host
// restatement mpcmp_clearance_config: the obstacle distance formulas, the pair rules and the ordering of ties (clearance_rule.hpp, plain C++, read by
// the host-only unit as well), the LDS budget and the launchers.
// The kernels themselves live in clearance.hip, a translation unit of their own: nothing here is a kernel, so including this header does not
// change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "../../include/mpcmp.h"
#include "clearance_rule.hpp"

namespace mpcmp {

constexpr int CLR_MAX_PTS = 4096;    // n_pts
constexpr int CLR_NT = 256;          // threads per workgroup of k_clearance

// a robot sphere as the kernel reads it (mpcmp_sphere plus its arm); table order = arm-major = the numbering of mpcmp_clearance.sphere
struct ClrSphere {
    double c[3], r;
    int joint, arm;
};

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
// the certified check (include/mpcmp_clearance_cert.h; the kernel is in clearance_cert.hip, the rule in clearance_cert.hpp); d_cert may be NULL
hipError_t clearance_cert_prepare();
hipError_t clearance_cert_launch(const ClrTables &t, int B, const double *d_sx, const double *d_sT, double margin, int self_gap, int n_start,
                                 int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st);
// keys [n_groups] scratch; chosen [n_groups].  d_clr and d_lim may each be NULL (that test is skipped); lim_mask: the bits of mpcmp_limits.status that
// make a member inadmissible (MPCMP_LIM_NAN always does)
hipError_t select_launch(int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr, const mpcmp_limits *d_lim, int lim_mask,
                         const int *d_group, int n_groups, unsigned long long *d_keys, int *d_chosen, hipStream_t st);

}  // namespace mpcmp
