// moving_cert.hpp — what the certified check in a moving world (include/mpcmp_moving_cert.h) shares between its entry points (mpcmp.hip) and its
// kernel (moving_cert.hip): the per-problem times and the launchers.  The rule is moving_cert_rule.hpp (plain C++, read by the host statement of
// model_host.cpp as well).  Nothing here is a kernel, so including this header does not change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include "moving.hpp"

namespace mpcmp {

// B finished plans on their own clock with their start times, waits and holds (each [B] or NULL: 0)
struct MvcPlans {
    const double *d_sx, *d_sT, *d_t_start, *d_wait, *d_hold;
};

hipError_t moving_cert_prepare();       // the kernel's dynamic-LDS ceiling; called by a context's first call
hipError_t moving_cert_launch(const ClrTables &t, const MvTracks &trk, const MvcPlans &p, int B, double margin, int self_gap, int n_start, int n_rest,
                              int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st);

}  // namespace mpcmp
