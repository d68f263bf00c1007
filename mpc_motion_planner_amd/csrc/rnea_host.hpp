// rnea_host.hpp — the Newton-Euler recursion in plain host C++, for the host statements of the checkers
// (mpcmp_limits_config, mpcmp_retime_one, mpcmp_retime_route_one, mpcmp_limits_retimed_one), which run without a context and without a GPU.
#pragma once
#include <cmath>
#include "../../include/mpcmp.h"

namespace mpcmp_host {

struct H3 { double x, y, z; };
inline H3 h3(const double *p) { return {p[0], p[1], p[2]}; }
inline H3 operator+(H3 a, H3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline H3 operator*(double s, H3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline H3 cr(H3 a, H3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline H3 mv(const double *R, H3 v) { return {R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z}; }
inline H3 mtv(const double *R, H3 v) { return {R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z}; }

// the Newton-Euler recursion of rnea_dir (rbd_device.hpp) without its tangent, in plain host C++
inline void rnea_host(const mpcmp_model &M, const double *q, const double *v, const double *a, double *tau) {
    double R[7][9];
    H3 F[7], Nn[7], w = {0, 0, 0}, wd = {0, 0, 0}, al = {-M.gravity[0], -M.gravity[1], -M.gravity[2]};
    for (int i = 0; i < 7; i++) {
        const double s = std::sin(q[i]), c = std::cos(q[i]), *A = M.R0[i];
        for (int r = 0; r < 3; r++) { R[i][3 * r] = A[3 * r] * c + A[3 * r + 1] * s; R[i][3 * r + 1] = -A[3 * r] * s + A[3 * r + 1] * c; R[i][3 * r + 2] = A[3 * r + 2]; }
        const H3 p = h3(M.p[i]), cm = h3(M.com[i]);
        const H3 u = mtv(R[i], w), ud = mtv(R[i], wd);
        const H3 bb = al + cr(wd, p) + cr(w, cr(w, p));
        const H3 wn = {u.x, u.y, u.z + v[i]};
        const H3 wdn = {ud.x + u.y * v[i], ud.y - u.x * v[i], ud.z + a[i]};
        const H3 aln = mtv(R[i], bb);
        const H3 acc = aln + cr(wdn, cm) + cr(wn, cr(wn, cm));
        F[i] = M.mass[i] * acc;
        Nn[i] = mv(M.I[i], wdn) + cr(wn, mv(M.I[i], wn));
        w = wn; wd = wdn; al = aln;
    }
    H3 f = {0, 0, 0}, n = {0, 0, 0};
    for (int i = 6; i >= 0; i--) {
        H3 fi = F[i], ni = Nn[i] + cr(h3(M.com[i]), F[i]);
        if (i < 6) {
            const H3 gf = mv(R[i + 1], f), gn = mv(R[i + 1], n);
            fi = fi + gf; ni = ni + gn + cr(h3(M.p[i + 1]), gf);
        }
        f = fi; n = ni;
        tau[i] = n.z;
    }
}

}  // namespace mpcmp_host
