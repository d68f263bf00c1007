// frame_rule.hpp — the part of the frame rule (include/mpcmp_frame.h) that is plain arithmetic: what a camera and a pad must satisfy, one entry of
// the filter table, the world point of a pixel, the class of a point and the carve test of a voxel.  Plain C++, so that the host-only unit
// (model_host.cpp) reads the same source as the kernels of frame.hip; frame.hpp includes it.  Nothing here is a kernel.
#pragma once
#include <cmath>
#include "clearance_cert.hpp"
#include "field_rule.hpp"

namespace mpcmp {

constexpr int FRM_MAX_SPH = 2 * CLR_MAX_SPH;      // both arms' tables
constexpr int FRM_MAX_PIXELS = MPCMP_FRAME_MAX_PIXELS;
// the classes in the order of their tests = the order of the counts in mpcmp_frame_stats behind n_in
enum { FRM_INVALID = 0, FRM_OUTSIDE = 1, FRM_ROBOT = 2, FRM_MARKED = 3 };

MPCMP_HD bool frm_pad_ok(double pad) { return fld_finite(pad) && pad >= 0.0; }

MPCMP_HD bool frm_camera_ok(const mpcmp_camera &c) {
    for (int i = 0; i < 9; i++) if (!fld_finite(c.R[i])) return false;
    for (int i = 0; i < 3; i++) if (!fld_finite(c.t[i])) return false;
    if (!fld_finite(c.fx) || !fld_finite(c.fy) || !fld_finite(c.cx) || !fld_finite(c.cy) || !fld_finite(c.depth_scale) || !fld_finite(c.z_min) ||
        !fld_finite(c.z_max)) return false;
    if (c.width < 1 || c.height < 1 || (long long)c.width * c.height > FRM_MAX_PIXELS) return false;
    return c.fx > 0.0 && c.fy > 0.0 && c.depth_scale > 0.0 && c.z_min >= 0.0 && c.z_min <= c.z_max;
}

// two grids are the same grid (MPCMP_FRAME_KEEP): origin, h and n; the pad word is not part of it
MPCMP_HD bool frm_same_grid(const mpcmp_field_desc &a, const mpcmp_field_desc &b) {
    for (int d = 0; d < 3; d++) if (a.origin[d] != b.origin[d] || a.n[d] != b.n[d]) return false;
    return a.h == b.h;
}

// one entry of the filter table, e [4] = c_s (3), R_s^2: F the world frame of the sphere's joint (cert_frames), c its centre in that frame
MPCMP_HD void frm_entry(const double *F, const double *c, double r, double pad, double *e) {
    cert_centre(F, c, e);
    const double R = r + pad;
    e[3] = R * R;
}

// |x - c_s|^2 <= R_s^2 for some s of the table tab [ns][4]
MPCMP_HD bool frm_in_robot(const double *tab, int ns, double x, double y, double z) {
    bool in = false;
    for (int s = 0; s < ns; s++) {
        const double dx = x - tab[4 * s], dy = y - tab[4 * s + 1], dz = z - tab[4 * s + 2];
        in = in || (dx * dx + dy * dy + dz * dz <= tab[4 * s + 3]);
    }
    return in;
}

// the class of the point x as one integer: the linear index of its voxel (>= 0) for FRM_MARKED, -1 - class for the other three
MPCMP_HD int frm_classify(const mpcmp_field_desc &g, const double *tab, int ns, const double *x) {
    if (!fld_finite(x[0]) || !fld_finite(x[1]) || !fld_finite(x[2])) return -1 - FRM_INVALID;
    const int v = fld_point_voxel(g, x);
    if (v < 0) return -1 - FRM_OUTSIDE;
    return frm_in_robot(tab, ns, x[0], x[1], x[2]) ? -1 - FRM_ROBOT : v;
}
MPCMP_HD int frm_class_of(int code) { return code >= 0 ? FRM_MARKED : -1 - code; }

// The world point of pixel (row v, column u) whose depth word converts to d; raw_ok: the word passed the test of its type (U16: d != 0, F32: d
// finite and > 0).  false: the pixel is INVALID
MPCMP_HD bool frm_pixel(const mpcmp_camera &c, int u, int v, double d, bool raw_ok, double *x) {
    if (!raw_ok) return false;
    const double z = d * c.depth_scale;
    if (z < c.z_min || z > c.z_max) return false;
    const double p[3] = {z * ((double)u - c.cx) / c.fx, z * ((double)v - c.cy) / c.fy, z};
    for (int r = 0; r < 3; r++) x[r] = c.R[3 * r] * p[0] + c.R[3 * r + 1] * p[1] + c.R[3 * r + 2] * p[2] + c.t[r];
    return true;
}
MPCMP_HD bool frm_raw_ok_u16(unsigned short d) { return d != 0; }
MPCMP_HD bool frm_raw_ok_f32(float d) { return fld_finite((double)d) && d > 0.0f; }

// the carve test of the voxel with the linear index `idx`: its centre lies in a filter sphere
MPCMP_HD bool frm_carved(const mpcmp_field_desc &g, const double *tab, int ns, int idx) {
    const int i = idx % g.n[0], j = idx / g.n[0] % g.n[1], k = idx / g.n[0] / g.n[1];
    return frm_in_robot(tab, ns, g.origin[0] + g.h * ((double)i + 0.5), g.origin[1] + g.h * ((double)j + 0.5), g.origin[2] + g.h * ((double)k + 0.5));
}

}  // namespace mpcmp
