// clearance.hpp — what the clearance checker shares between the host entry points (mpcmp.hip), its kernels (clearance.hip) and the host
// restatement mpcmp_clearance_config: the obstacle distance formulas, the pair rules and the ordering of ties (clearance_rule.hpp, plain C++, read by
// the host-only unit as well), the LDS layouts (clearance_lds.hpp) and the launchers.
// The kernels themselves live in clearance.hip, a translation unit of their own: nothing here is a kernel, so including this header does not
// change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include "../../include/mpcmp.h"
#include "clearance_rule.hpp"
#include "clearance_lds.hpp"

namespace mpcmp {

constexpr int CLR_MAX_PTS = 4096;    // n_pts
constexpr int CLR_NT = 256;          // threads per workgroup of k_clearance

// a robot sphere as the kernel reads it (mpcmp_sphere plus its arm); table order = arm-major = the numbering of mpcmp_clearance.sphere
struct ClrSphere {
    double c[3], r;
    int joint, arm;
};

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
// The certified check, without a timeline (include/mpcmp_clearance_cert.h) and with one (include/mpcmp_moving_cert.h): the kernel is in
// clearance_cert.hip, the rule in clearance_cert.hpp and moving_cert_rule.hpp.  B finished plans on their own clock with their start times, waits
// and holds (each [B] or NULL: 0); trk (moving.hpp) NULL: the static certificate, which reads d_sx and d_sT only; d_cert may be NULL
struct MvTracks;
struct CertPlans {
    const double *d_sx, *d_sT, *d_t_start, *d_wait, *d_hold;
};
hipError_t clearance_cert_prepare();    // the dynamic-LDS ceilings of both instantiations
hipError_t clearance_cert_launch(const ClrTables &t, const MvTracks *trk, const CertPlans &p, int B, double margin, int self_gap, int n_start,
                                 int n_rest, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st);
// keys [n_groups] scratch; chosen [n_groups].  d_clr and d_lim may each be NULL (that test is skipped); lim_mask: the bits of mpcmp_limits.status that
// make a member inadmissible (MPCMP_LIM_NAN always does)
hipError_t select_launch(int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr, const mpcmp_limits *d_lim, int lim_mask,
                         const int *d_group, int n_groups, unsigned long long *d_keys, int *d_chosen, hipStream_t st);

}  // namespace mpcmp
