// frame.hpp — what the frame family (include/mpcmp_frame.h) shares between the host entry points (mpcmp.hip) and its kernels (frame.hip): the
// launchers and what they take.  The rule's arithmetic is in frame_rule.hpp (plain C++, read by the host statements of model_host.cpp as well).
// The kernels live in frame.hip, a translation unit of their own: nothing here is a kernel, so including this header does not change what any
// other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "field.hpp"
#include "frame_rule.hpp"

namespace mpcmp {

constexpr int FRM_NT = 256;          // threads per workgroup of the marker and the carver
// the sources of k_frame_mark: a cloud of doubles, a depth image of either type
enum { FRM_SRC_POINTS = 0, FRM_SRC_U16 = 1, FRM_SRC_F32 = 2 };

// the capture posture, passed to k_frame_spheres by value
struct FrmPosture { double q[14]; };
// the filter in force for one call: d_tab [ns][4] = c_s, R_s^2 (context-owned, FRM_MAX_SPH entries); ns == 0: no filter, d_tab is not read
struct FrmFilter {
    const double *d_tab;
    int ns;
};

// the chain at q for each arm, then one lane per sphere: d_tab [t.n_sph[0] + t.n_sph[1]][4]
hipError_t frame_spheres_launch(const ClrTables &t, const FrmPosture &q, double pad, double *d_tab, hipStream_t st);
// zero *d_stats, zero the occupancy unless `keep`, classify and mark the n items of `d_src` (src: points [n][3], or the pixels of cam, n = width x
// height); cam is read for the depth sources only
hipError_t frame_mark_launch(const FldArrays &f, int src, int n, const void *d_src, const mpcmp_camera *cam, const FrmFilter &flt, bool keep,
                             mpcmp_frame_stats *d_stats, hipStream_t st);
// zero *d_stats and clear the occupied voxels whose centre lies in a filter sphere
hipError_t frame_carve_launch(const FldArrays &f, const FrmFilter &flt, mpcmp_frame_stats *d_stats, hipStream_t st);

}  // namespace mpcmp
