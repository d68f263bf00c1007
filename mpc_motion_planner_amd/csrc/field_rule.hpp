// field_rule.hpp — the part of the voxel-world rule (include/mpcmp_field.h) that is plain arithmetic: what a grid must satisfy, the voxel of a
// point, one output of a min-plus sweep of the distance transform, the distance of a world point and the merge of two clearance records.  Plain
// C++, so that the host-only unit (model_host.cpp) reads the same source as the kernels of field.hip; field.hpp includes it.  Nothing here is a
// kernel.
#pragma once
#include <cmath>
#include "clearance_rule.hpp"

namespace mpcmp {

constexpr int FLD_MAX_DIM = MPCMP_FIELD_MAX_DIM;
constexpr int FLD_MAX_VOXELS = MPCMP_FIELD_MAX_VOXELS;
// The "infinity" of the transform's passes: finite, so that g + (j - j')^2 cannot overflow (FLD_INF + 1023^2 < 2^31), and above every true value
// (3 x 1023^2 < 2^22).  Only the last pass's write turns it into MPCMP_FIELD_EMPTY
constexpr unsigned FLD_INF = 0x3FFFFFFFu;

MPCMP_HD bool fld_finite(double x) { return x - x == 0.0; }

MPCMP_HD bool fld_desc_ok(const mpcmp_field_desc &g) {
    long long nv = 1;
    for (int d = 0; d < 3; d++) {
        if (g.n[d] < 1 || g.n[d] > FLD_MAX_DIM || !fld_finite(g.origin[d])) return false;
        nv *= g.n[d];
    }
    return nv <= FLD_MAX_VOXELS && fld_finite(g.h) && g.h > 0.0;
}
MPCMP_HD int fld_voxels(const mpcmp_field_desc &g) { return g.n[0] * g.n[1] * g.n[2]; }

// the linear index of the voxel that contains the point p, -1 for a point that is not finite or lies outside the grid (0 <= u < n, half open)
MPCMP_HD int fld_point_voxel(const mpcmp_field_desc &g, const double *p) {
    int v[3];
    for (int d = 0; d < 3; d++) {
        const double u = (p[d] - g.origin[d]) / g.h;
        if (!(u >= 0.0 && u < (double)g.n[d])) return -1;            // (a NaN fails both)
        v[d] = (int)floor(u);
    }
    return (v[2] * g.n[1] + v[1]) * g.n[0] + v[0];
}

// One step of a min-plus sweep: the running minimum `best` (at most FLD_INF) of an output joined with the entry g that lies d places away,
// min(best, g + d^2).  |d| < 2^11 and g <= FLD_INF, so nothing overflows; integer arithmetic only
MPCMP_HD unsigned fld_step(unsigned best, unsigned g, int d) {
#ifdef __HIP_DEVICE_COMPILE__
    const unsigned v = g + (unsigned)__mul24(d, d);                      // (one v_mad_i32_i24)
#else
    const unsigned v = g + (unsigned)(d * d);
#endif
    return v < best ? v : best;
}
// one output of a sweep along a line of n entries: min over k of g[k] + (j - k)^2, kept at FLD_INF
MPCMP_HD unsigned fld_minplus(const unsigned *g, int n, int j) {
    unsigned best = FLD_INF;
    for (int k = 0; k < n; k++) best = fld_step(best, g[k], j - k);
    return best;
}

// sd_field of the world point x and the voxel read (include/mpcmp_field.h, "Distance")
MPCMP_HD double fld_sd(const mpcmp_field_desc &g, const unsigned *d2, double x, double y, double z, int *voxel) {
    const double p[3] = {x, y, z};
    double e2 = 0.0;
    int v[3];
    for (int d = 0; d < 3; d++) {
        const double u = (p[d] - g.origin[d]) / g.h;
        const double uc = fmin(fmax(u, 0.0), (double)g.n[d]);
        int i = (int)floor(uc);
        if (i > g.n[d] - 1) i = g.n[d] - 1;
        const double e = uc - ((double)i + 0.5);
        e2 += e * e;
        v[d] = i;
    }
    const int idx = (v[2] * g.n[1] + v[1]) * g.n[0] + v[0];
    *voxel = idx;
    const unsigned q = d2[idx];
    if (q == MPCMP_FIELD_EMPTY) return INFINITY;
    return g.h * (sqrt((double)q) - sqrt(e2) - 0.8660254037844386);      // sqrt(3) / 2
}

// Ties of d_min of the field check: lowest sample, then lowest sphere = the order of clr_pack(sample, sphere, 0, 0)

// two records of one problem as one (include/mpcmp_field.h, mpcmp_clearance_merge_batch); *source: where d_min came from
MPCMP_HD mpcmp_clearance fld_merge(const mpcmp_clearance &a, const mpcmp_clearance &b, int *source) {
    mpcmp_clearance o;
    o.d_min = INFINITY; o.t_min = -1.0; o.t_first = -1.0; o.sphere = -1; o.other = 0;
    o.n_hit = a.n_hit + b.n_hit; o.status = a.status | b.status;
    *source = 0;
    if (a.sphere >= 0) { o.d_min = a.d_min; o.t_min = a.t_min; o.sphere = a.sphere; o.other = a.other; }
    if (b.sphere >= 0 && (a.sphere < 0 || b.d_min < a.d_min)) { o.d_min = b.d_min; o.t_min = b.t_min; o.sphere = b.sphere; o.other = b.other; *source = 1; }
    if (a.t_first >= 0.0) o.t_first = a.t_first;
    if (b.t_first >= 0.0 && (o.t_first < 0.0 || b.t_first < o.t_first)) o.t_first = b.t_first;
    if (o.status & MPCMP_CLR_NAN) { o.d_min = NAN; o.t_min = -1.0; o.t_first = -1.0; o.sphere = -1; o.other = 0; o.n_hit = 0; *source = 0; }
    return o;
}

}  // namespace mpcmp
