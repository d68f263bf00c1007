// clearance_cert.hpp — the rule of the certified clearance check (include/mpcmp_clearance_cert.h) as host/device functions: the geometry of an
// interval, the Bezier deviation of a joint, the reach table, the frames of one arm, the decision and the tie keys.  The kernel (clearance_cert.hip)
// and the host statement mpcmp_clearance_certified_one (model_host.cpp) both run this source.  Plain C++: no HIP header, and nothing here is a kernel.
#pragma once
#include <cmath>
#include "clearance_rule.hpp"
#include "plan_interp.hpp"

namespace mpcmp {

constexpr int CERT_CAP = MPCMP_CLR_CERT_CAPACITY;   // intervals per level
constexpr int CERT_SPLIT = CERT_CAP / 2;            // intervals of one level that may be split
constexpr int CERT_MAX_DEPTH = 16;

// Interval (l, i) of n0 = nseg n_start level-0 intervals: its segment, its ends and midpoint in normalised time, its width.  Every quotient has an
// exact numerator and an exact denominator (below 2^30), so a time is the correctly rounded value of its fraction however it is reached.
struct CertInterval {
    int seg;
    double ta, tm, tb, h;
};
MPCMP_HD CertInterval cert_interval(int n0, int n_start, int l, int i) {
    CertInterval v;
    const double den = (double)n0 * (double)(1 << l);
    v.seg = (i >> l) / n_start;
    v.ta = (double)i / den;
    v.tb = (double)(i + 1) / den;
    v.tm = (double)(2 * i + 1) / (2.0 * den);
    v.h = 1.0 / den;
    return v;
}

// The order of midpoints across levels as an integer: t_m = key / (n0 2^17), key = (2 i + 1) 2^(16 - l) < 2^29; distinct intervals have distinct keys
MPCMP_HD unsigned cert_tkey(int l, int i) { return (unsigned)(2 * i + 1) << (CERT_MAX_DEPTH - l); }
MPCMP_HD double cert_time(int n0, unsigned tkey) { return (double)tkey / ((double)n0 * 131072.0); }
constexpr unsigned CERT_NO_TIME = 0xFFFFFFFFu;

// Ties of d_min: lowest midpoint, then lowest sphere, then obstacles before robot pairs, then lowest index = the order of this key (clr_pack with the
// midpoint key in place of the sample).  Ties of d_lower: lowest midpoint = the same key with the low 16 bits 0
MPCMP_HD unsigned long long cert_key(unsigned tkey, int sphere, int robot, int idx) {
    return ((unsigned long long)tkey << 16) | ((unsigned long long)sphere << 9) | ((unsigned long long)robot << 8) | (unsigned long long)idx;
}
constexpr unsigned long long CERT_NO_PAIR = ~0ull;
MPCMP_HD bool cert_better(double d, unsigned long long k, double bd, unsigned long long bk) { return d < bd || (d == bd && k < bk); }

// dev of one joint column on an interval, and q(t_m): C points at the column in node 0, `stride` doubles lie between two nodes
MPCMP_HD double cert_deviation(const double *C, int stride, int nseg, const CertInterval &v, double *q_m) {
    double W[4];
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.tm, W);
    const double qm = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.ta, W);
    const double b0 = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_derivative_on_segment(nseg, v.seg, v.ta, W);
    const double b1 = b0 + (v.h / 3.0) * mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_on_segment(nseg, v.seg, v.tb, W);
    const double b3 = mpcmp_plan::interp_channel(C, stride, v.seg, W);
    mpcmp_plan::lagrange_derivative_on_segment(nseg, v.seg, v.tb, W);
    const double b2 = b3 - (v.h / 3.0) * mpcmp_plan::interp_channel(C, stride, v.seg, W);
    *q_m = qm;
    return fmax(fmax(fabs(b0 - qm), fabs(b1 - qm)), fmax(fabs(b2 - qm), fabs(b3 - qm)));
}

// reach [7] of a sphere with the centre c on joint `joint` of the arm whose joint offsets are p(k) = P[pstride k .. + 3]: entries above `joint` are 0,
// so that D_s is one sum over the arm's seven deviations
MPCMP_HD void cert_reach(const double *P, int pstride, int joint, const double *c, double *reach) {
    double r = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    for (int i = 6; i > joint; i--) reach[i] = 0.0;
    for (int i = joint; i >= 0; i--) {
        reach[i] = r;
        const double *p = P + pstride * i;
        r += sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    }
}
MPCMP_HD double cert_motion(const double *reach, const double *dev) {
    double D = 0.0;
    for (int i = 0; i < 7; i++) D += reach[i] * dev[i];
    return D;
}

// World rotation and origin of the seven joint frames of one arm, F [7][12] = Rw (9), pw (3), from its placements M [7][12] = R0 (9), p (3) and the
// sines and cosines SC [7][2] of its joints: p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i)
MPCMP_HD void cert_frames(const double *M, const double *SC, double *F) {
    double Rw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pw[3] = {0, 0, 0};
    PLAN_UNROLL
    for (int i = 0; i < 7; i++) {
        const double *A = M + 12 * i;
        const double s = SC[2 * i], c = SC[2 * i + 1];
        double R[9], Rn[9];
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) {
            R[3 * r] = A[3 * r] * c + A[3 * r + 1] * s;
            R[3 * r + 1] = -A[3 * r] * s + A[3 * r + 1] * c;
            R[3 * r + 2] = A[3 * r + 2];
        }
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) pw[r] += Rw[3 * r] * A[9] + Rw[3 * r + 1] * A[10] + Rw[3 * r + 2] * A[11];
        PLAN_UNROLL
        for (int r = 0; r < 3; r++)
            PLAN_UNROLL
            for (int c2 = 0; c2 < 3; c2++) Rn[3 * r + c2] = Rw[3 * r] * R[c2] + Rw[3 * r + 1] * R[3 + c2] + Rw[3 * r + 2] * R[6 + c2];
        PLAN_UNROLL
        for (int k = 0; k < 9; k++) { Rw[k] = Rn[k]; F[12 * i + k] = Rn[k]; }
        PLAN_UNROLL
        for (int r = 0; r < 3; r++) F[12 * i + 9 + r] = pw[r];
    }
}
// world centre of a sphere with the centre c in the frame F [12] of its joint
MPCMP_HD void cert_centre(const double *F, const double *c, double *w) {
    w[0] = F[9] + F[0] * c[0] + F[1] * c[1] + F[2] * c[2];
    w[1] = F[10] + F[3] * c[0] + F[4] * c[1] + F[5] * c[2];
    w[2] = F[11] + F[6] * c[0] + F[7] * c[1] + F[8] * c[2];
}

// the decision of one interval (the order is part of the rule; a NaN never certifies: it ends as UNDECIDED or is split)
enum { CERT_HIT = 0, CERT_CLEAR = 1, CERT_UNDECIDED = 2, CERT_SPLIT_IT = 3 };
MPCMP_HD int cert_decide(double d_mid, double L, double margin, int l, int max_depth) {
    if (d_mid < margin) return CERT_HIT;
    if (L >= margin) return CERT_CLEAR;
    if (l == max_depth) return CERT_UNDECIDED;
    return CERT_SPLIT_IT;
}

}  // namespace mpcmp
