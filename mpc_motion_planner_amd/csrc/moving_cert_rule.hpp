// moving_cert_rule.hpp — what the certified check in a moving world (include/mpcmp_moving_cert.h) adds to the static certificate
// (clearance_cert.hpp) and to the tracks (moving_rule.hpp): the timeline of wait, motion and hold, the phase geometry of an interval, the
// conversion of a midpoint key to a record time, and the displacement bound E_k of a track on an interval.  The kernel (k_clearance_cert with a
// timeline, clearance_cert.hip) and the host statement mpcmp_clearance_certified_timed_one (model_host.cpp) both run this source.  Plain C++: no HIP header, and nothing here is a kernel.
#pragma once
#include <cmath>
#include "clearance_cert.hpp"
#include "moving_rule.hpp"
#include "plan_interp.hpp"

namespace mpcmp {

enum { MVC_WAIT = 0, MVC_MOTION = 1, MVC_HOLD = 2 };

// durations a record can be made of: finite, and the rests not negative
MPCMP_HD bool mvc_times_ok(double T, double t_start, double w, double h) {
    return mv_finite(T) && mv_finite(t_start) && mv_finite(w) && mv_finite(h) && w >= 0.0 && h >= 0.0;
}

// The timeline of one problem: level-0 counts of the three phases, their durations, and tau0 = t_start - w, the world time of the record time 0
struct MvcTimeline {
    int n_w, n_m, n_h, n0;
    double w, T, h, tau0;
};
MPCMP_HD MvcTimeline mvc_timeline(int nseg, int n_start, int n_rest, double T, double t_start, double w, double h) {
    MvcTimeline tl;
    tl.n_w = w > 0.0 ? n_rest : 0; tl.n_m = nseg * n_start; tl.n_h = h > 0.0 ? n_rest : 0;
    tl.n0 = tl.n_w + tl.n_m + tl.n_h;
    tl.w = w; tl.T = T; tl.h = h; tl.tau0 = t_start - w;
    return tl;
}

// the phase of the level-0 interval g: its first level-0 index, its level-0 count, the record time of its start and its duration
struct MvcPhase {
    int phase, first, n_p;
    double base, len;
};
MPCMP_HD MvcPhase mvc_phase(const MvcTimeline &tl, int g) {
    MvcPhase p;
    if (g < tl.n_w) { p.phase = MVC_WAIT; p.first = 0; p.n_p = tl.n_w; p.base = 0.0; p.len = tl.w; }
    else if (g < tl.n_w + tl.n_m) { p.phase = MVC_MOTION; p.first = tl.n_w; p.n_p = tl.n_m; p.base = tl.w; p.len = tl.T; }
    else { p.phase = MVC_HOLD; p.first = tl.n_w + tl.n_m; p.n_p = tl.n_h; p.base = tl.w + tl.T; p.len = tl.h; }
    return p;
}

// Interval (l, i) of the timeline: its phase, its place INSIDE the phase as an interval of the static rule (v: fractions of the phase, and for a
// motion interval its segment), and its ends and midpoint on the record clock
struct MvcInterval {
    int phase;
    CertInterval v;
    double ta, tm, tb;
};
MPCMP_HD MvcInterval mvc_interval(const MvcTimeline &tl, int n_start, int l, int i) {
    const MvcPhase p = mvc_phase(tl, i >> l);
    MvcInterval r;
    r.phase = p.phase;
    r.v = cert_interval(p.n_p, p.phase == MVC_MOTION ? n_start : p.n_p, l, i - (p.first << l));
    r.ta = p.base + r.v.ta * p.len; r.tm = p.base + r.v.tm * p.len; r.tb = p.base + r.v.tb * p.len;
    return r;
}
// the record time of a midpoint key (cert_tkey with the global i): key / 2^17 is the midpoint in level-0 intervals, so its integer part is g
MPCMP_HD double mvc_time(const MvcTimeline &tl, unsigned tkey) {
    const MvcPhase p = mvc_phase(tl, (int)(tkey >> (CERT_MAX_DEPTH + 1)));
    return p.base + ((double)(tkey - ((unsigned)p.first << (CERT_MAX_DEPTH + 1))) / ((double)p.n_p * 131072.0)) * p.len;
}

MPCMP_HD double mvc_dist(const double *a, const double *b) {
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return sqrt(x * x + y * y + z * z);
}
// p_m [3] = the offset of the track P [n_key][3] at tau_m, and E_k: the largest distance from p_m of the track on [tau_a, tau_b], taken over the
// polyline's vertices there: both ends and every key strictly or not inside (a key on an end repeats an end point)
MPCMP_HD double mvc_track_bound(const double *P, int n_key, double t0, double dt, double tau_a, double tau_m, double tau_b, double *p_m) {
    mv_offset(P, mv_place(n_key, t0, dt, tau_m), p_m);
    if (n_key < 2) return 0.0;
    double x[3];
    mv_offset(P, mv_place(n_key, t0, dt, tau_a), x);
    double E = mvc_dist(x, p_m);
    mv_offset(P, mv_place(n_key, t0, dt, tau_b), x);
    E = fmax(E, mvc_dist(x, p_m));
    const double ua = fmin(fmax((tau_a - t0) / dt, 0.0), (double)(n_key - 1)), ub = fmin(fmax((tau_b - t0) / dt, 0.0), (double)(n_key - 1));
    const int jb = (int)floor(ub);
    for (int j = (int)ceil(ua); j <= jb; j++) E = fmax(E, mvc_dist(P + 3 * j, p_m));
    return E;
}

}  // namespace mpcmp
