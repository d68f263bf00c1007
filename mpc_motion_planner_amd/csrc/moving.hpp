// moving.hpp — what the checks in a moving world (include/mpcmp_moving.h) share between the host entry points (mpcmp.hip) and their kernels
// (moving.hip): the track table as a kernel reads it, the plan with its profile and start times, the LDS budget and the launchers.  The rule's
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

// dynamic LDS of the three kernels in bytes: the tables and the chunk of k_clearance, the clock of a chunk's samples and (k_start_delay) K delays
inline size_t mv_lds_bytes(int narm, int N, int nsph, int n_obs, int chunk, int K) {
    const size_t dbl = (size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 14 +
                       (size_t)chunk * narm * 84 + (size_t)chunk * nsph * 3 + (size_t)3 * chunk + (size_t)3 * K;
    const size_t ints = (size_t)2 * nsph + (size_t)3 * n_obs + (size_t)3 * chunk;
    return dbl * sizeof(double) + (ints + 1) / 2 * 2 * sizeof(int);
}

hipError_t moving_prepare();        // the kernels' dynamic-LDS ceilings; called by a context's first call of this family
hipError_t clearance_timed_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int n_pts, double margin, int self_gap,
                                  mpcmp_clearance *d_out, hipStream_t st);
hipError_t start_delay_launch(const ClrTables &t, const MvTracks &trk, const MvPlans &p, int B, int K, const double *d_delays, int check_wait,
                              int n_pts, double margin, int self_gap, double *d_min_all, mpcmp_start_delay *d_out, hipStream_t st);
hipError_t sphere_tracks_launch(const ClrTables &t, const MvPlans &p, int B, double t0, double dt, int n_key, double *d_out, hipStream_t st);

}  // namespace mpcmp
