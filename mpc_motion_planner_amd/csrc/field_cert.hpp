// field_cert.hpp — what the certified clearance check against a voxel world (include/mpcmp_field_cert.h) shares between the host entry points
// (mpcmp.hip) and its kernels (field_cert.hip): the launchers.  The rule is field_cert_rule.hpp on top of clearance_cert.hpp and field_rule.hpp.
// The kernels live in field_cert.hip, a translation unit of their own: nothing here is a kernel, so including this header does not change what any
// other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include "field.hpp"
#include "field_cert_rule.hpp"

namespace mpcmp {

hipError_t field_cert_prepare();    // the dynamic-LDS ceiling of k_clearance_cert_field; called by a context's first certified field check
// t.d_obs / n_obs are not read; d_cert may be NULL
hipError_t clearance_cert_field_launch(const ClrTables &t, const FldArrays &f, int B, const double *d_sx, const double *d_sT, double margin, int n_start,
                                       int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st);
hipError_t clearance_cert_merge_launch(int B, const mpcmp_clearance_cert *d_a, const mpcmp_clearance_cert *d_b, mpcmp_clearance_cert *d_out,
                                       hipStream_t st);

}  // namespace mpcmp
