// field.hpp — what the voxel-world checks (include/mpcmp_field.h) share between the host entry points (mpcmp.hip) and their kernels (field.hip):
// the field as a kernel reads it and the launchers (the LDS layout is clearance_lds.hpp).  The rule's arithmetic is in field_rule.hpp (plain C++, read by the host
// statements of model_host.cpp as well).  The kernels live in field.hip, a translation unit of their own: nothing here is a kernel, so including
// this header does not change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "clearance.hpp"
#include "field_rule.hpp"

namespace mpcmp {

// the transform's tile: FLD_TILE entries of LDS (64 KB) hold tx neighbouring columns of one whole line each, tx a power of two in [1, 64]; a line
// of 1024 entries leaves 16 columns
constexpr int FLD_TILE = 16384;
constexpr int FLD_NT = 256;          // threads per workgroup of the transform's passes

// the field in force: the grid, its device arrays (each of fld_voxels(desc) entries) and the scratch of the transform
struct FldArrays {
    mpcmp_field_desc desc;
    unsigned char *d_occ;
    unsigned *d_d2, *d_tmp;
};

hipError_t field_prepare();         // the check kernel's dynamic-LDS ceiling; called by a context's first field check
// zero the occupancy and mark the voxels of n_points points (device) in it
hipError_t field_mark_launch(const FldArrays &f, int n_points, const double *d_points, hipStream_t st);
// d_occ -> d_d2 in three passes through d_tmp
hipError_t field_build_launch(const FldArrays &f, hipStream_t st);
// t.d_obs / n_obs are not read
hipError_t clearance_field_launch(const ClrTables &t, const FldArrays &f, int B, const double *d_sx, const double *d_sT, int n_pts, double margin,
                                  mpcmp_clearance *d_out, hipStream_t st);
hipError_t clearance_merge_launch(int B, const mpcmp_clearance *d_a, const mpcmp_clearance *d_b, mpcmp_clearance *d_out, int *d_source, hipStream_t st);

}  // namespace mpcmp
