// moving.hpp — what the checks in a moving world (include/mpcmp_moving.h) share between the host entry points (mpcmp.hip) and their kernels
// (moving.hip): the track table as a kernel reads it, the plan with its profile and start times, and the launchers (the LDS layout is clearance_lds.hpp).  The rule's
// arithmetic is in moving_rule.hpp (plain C++, read by the host statements of model_host.cpp as well).  The kernels live in moving.hip, a translation
// unit of their own: nothing here is a kernel, so including this header does not change what any other translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "clearance.hpp"
#include "moving_rule.hpp"

namespace mpcmp {

// the track table in force beside ClrTables (which stays as it is): n_tracks == 0 is a world that stands still.  With one obstacle set per problem
// (ClrTables::obs_stride != 0) problem b reads set b of both arrays, otherwise set 0
struct MvTracks {
    const int *d_track_of;           // [n_sets][n_obs]
    const double *d_offsets;         // [n_sets][n_tracks][n_key][3]
    int n_tracks, n_key;
    double t0, dt;
};
// B finished plans, their retime profiles (or NULL) and start times (or NULL: 0)
struct MvPlans {
    const double *d_sx, *d_sT, *d_prof, *d_t_start;
    int n_grid;
};

hipError_t moving_prepare();        // the kernels' dynamic-LDS ceilings; called by a context's first call of this family
hipError_t clearance_timed_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int n_pts, double margin, int self_gap,
                                  mpcmp_clearance *d_out, hipStream_t st);
hipError_t start_delay_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int K, const double *d_delays, int check_wait,
                              int n_pts, double margin, int self_gap, double *d_min_all, mpcmp_start_delay *d_out, hipStream_t st);
hipError_t sphere_tracks_launch(const ClrTables &t, const MvPlans &p, int B, double t0, double dt, int n_key, double *d_out, hipStream_t st);

}  // namespace mpcmp
