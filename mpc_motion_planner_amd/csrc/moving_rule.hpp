// moving_rule.hpp — the part of the moving-world rule (include/mpcmp_moving.h) that is plain arithmetic: where a world time lies on a track, the
// offset there, where a sample of the running clock lies on the plan, and the record of a start-delay search from its runs' minima.  Plain C++, so
// that the host-only unit (model_host.cpp) reads the same source as the kernels of moving.hip; moving.hpp includes it.  Nothing here is a kernel.
#pragma once
#include <cmath>
#include "clearance_rule.hpp"
#include "profile_place.hpp"

namespace mpcmp {

constexpr int MV_MAX_TRACKS = MPCMP_MAX_TRACKS, MV_MAX_KEYS = MPCMP_MAX_TRACK_KEYS, MV_MAX_DELAYS = MPCMP_MAX_DELAYS;
constexpr int MV_MAX_GRID = 4096;      // n_grid of a profile (RT_MAX_GRID of retime.hpp, which the host-only unit cannot read)

MPCMP_HD bool mv_finite(double x) { return x - x == 0.0; }

// Where the world time tau (finite) lies on the clock t0 + k dt of n_key keys: the key k and the weight f of key k1 = k + 1 (k1 = k for one key,
// f = 0), so that p = (1 - f) P[k] + f P[k1]
struct MvPlace { int k, k1; double f; };
MPCMP_HD MvPlace mv_place(int n_key, double t0, double dt, double tau) {
    MvPlace w;
    if (n_key < 2) { w.k = 0; w.k1 = 0; w.f = 0.0; return w; }
    const double u = fmin(fmax((tau - t0) / dt, 0.0), (double)(n_key - 1));
    int k = (int)floor(u);
    if (k > n_key - 2) k = n_key - 2;
    w.k = k; w.k1 = k + 1; w.f = u - k;
    return w;
}
// the offset of the track P [n_key][3] at a place
MPCMP_HD void mv_offset(const double *P, const MvPlace &w, double *p) {
    for (int d = 0; d < 3; d++) p[d] = (1.0 - w.f) * P[3 * w.k + d] + w.f * P[3 * w.k1 + d];
}
// a track index as the checks read it: anything outside [0, n_tracks) stands still
MPCMP_HD int mv_track(int t, int n_tracks) { return (t >= 0 && t < n_tracks) ? t : -1; }

// the running time of a plan: the end of its profile pf [n + 1][2], or its own duration
MPCMP_HD double mv_run_time(const double *pf, int n, double T) { return pf ? pf[2 * n] : T; }
// sample i of n_pts on the running clock: its time t and the plan's normalised time s there
MPCMP_HD void mv_sample(const double *pf, int n, double T, double T_run, int i, int n_pts, double *t, double *s) {
    const double r = (double)i / n_pts;
    *t = r * T_run;
    *s = pf ? rc_place(pf, n, fmin(fmax(*t, 0.0), T_run), 0.5 / T, i == n_pts).s : r;
}
// the plan's normalised time at the running time t, clamped to the plan: held at s = 0 before its start and at s = 1 after its end
MPCMP_HD double mv_held_s(const double *pf, int n, double T, double T_run, double t) {
    if (!(t > 0.0)) return 0.0;
    if (!(t < T_run)) return 1.0;
    return pf ? rc_place(pf, n, t, 0.5 / T, false).s : fmin(t / T_run, 1.0);
}

// The record of a start-delay search from the K runs' smallest clearances dk (its own samples) and, with check_wait, the smallest clearances w0 of
// the start posture at the world times delays[k]: run k is joined with min(w0[0 .. k]).  d_all [K] or NULL receives the joined minima.
// (called by one thread / the host: a sequential pass, so the lowest index and the counts need no ordering rule)
MPCMP_HD mpcmp_start_delay mv_delay_record(int K, const double *delays, const double *dk, const double *w0, int check_wait, double margin,
                                           double *d_all) {
    mpcmp_start_delay r;
    r.delay = -1.0; r.d_min = -INFINITY; r.index = -1; r.n_clear = 0; r.status = 0; r.pad = 0;
    double wait = INFINITY;
    for (int k = 0; k < K; k++) {
        double d = dk[k];
        if (check_wait) { wait = fmin(wait, w0[k]); d = fmin(d, wait); }
        if (d_all) d_all[k] = d;
        if (!(d < margin)) {
            r.n_clear++;
            if (r.index < 0) { r.index = k; r.delay = delays[k]; r.d_min = d; }
        } else if (r.index < 0 && d > r.d_min) r.d_min = d;
    }
    if (r.index < 0) r.status = MPCMP_CLR_HIT;
    return r;
}
// ... and of a NaN plan
MPCMP_HD mpcmp_start_delay mv_delay_nan(int K, double *d_all) {
    mpcmp_start_delay r;
    r.delay = -1.0; r.d_min = NAN; r.index = -1; r.n_clear = 0; r.status = MPCMP_CLR_NAN; r.pad = 0;
    if (d_all) for (int k = 0; k < K; k++) d_all[k] = NAN;
    return r;
}

}  // namespace mpcmp
