// Host-side check of the node interpolant of a finished plan (mpc_motion_planner_amd/csrc/plan_interp.hpp), compiled and run by
// tests/test_plan_interp_host.py.  Prints "ok <nseg>" per discretisation or a diagnostic and exits non-zero.  Only finite times are tried: the
// conversion of a non-number to int is not defined on the host.
//
// The bounds, with u = 2^-53 (round to nearest) and S = sum_j |Lg[j]| of the weights at hand:
//   * a weight is three factors (xx - xi_k) / (xi_j - xi_k): the nodes and their differences are exact in binary, so a factor costs two roundings
//     (the subtraction, the division) and the product of the three two more (1.0 * f is exact): 8 roundings, |Lg_j - L_j(xx)| <= 8 u |L_j(xx)|.  The exact
//     L_j(xx) sum to 1 for every xx, and the check's own sum of four adds 3 roundings: |sum - 1| <= 11 u S, taken as 12 u S for the second-order terms.
//   * xx = 2 (t nseg - s) - 1: the product rounds once (<= u t nseg), the difference with the integer s and the doubling are exact, the last
//     subtraction rounds once (<= u |xx| <= u on the segment): the place on the plan is off by <= (2 u t nseg + u) / (2 nseg) <= 1.5 u |t| + u in time.
//   * a weighted sum of four is a dot product from 0.0: 4 roundings on top of the weights' 8, so 12 u sum_j |Lg_j c_j| <= 12 u S max|c|.
//   * the node times (s + f) / nseg round once; interpolating them at one of them must give that time back, the interpolant of a straight line
//     being the line: |result - t| <= (12 + 1) u S (data <= 1) + 1.5 u + u + u t  ->  (14 S + 4) u with one unit of S for the second-order terms.
//   * a cubic p(t) = sum a_i t^i evaluated by Horner's rule is off by <= 6 u A, A = sum |a_i| T^i with T = max(1, |t|) (three multiply-adds); its node
//     values carry that error, amplified by S; the place is off by <= 2.5 u T + u in time, times |p'| <= A1 = sum i |a_i| T^(i-1); the direct evaluation
//     compared against is off by 6 u A again:  |result - p(t)| <= u (18 S A + 6 A + 3.5 T A1), taken with 19 S A for the second-order terms.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../mpc_motion_planner_amd/csrc/plan_interp.hpp"

using namespace mpcmp_plan;

static const double U = 0.5 * DBL_EPSILON;

static int fail(const char *what, int nseg, double a = 0.0, double b = 0.0) { std::printf("FAIL nseg %d: %s (%.17g, %.17g)\n", nseg, what, a, b); return 1; }

static double abs_sum(const double *Lg) { return std::fabs(Lg[0]) + std::fabs(Lg[1]) + std::fabs(Lg[2]) + std::fabs(Lg[3]); }
static bool is_unit(const double *Lg, int j) {
    for (int k = 0; k < 4; k++) if (Lg[k] != (k == j ? 1.0 : 0.0)) return false;
    return true;
}

// channel c of the test plan is the cubic with these coefficients (of the normalised time)
static const double COEF[4][4] = {{0.3, -1.1, 2.0, -0.7}, {-2.5, 0.0, 0.9, 1.6}, {1.0, 4.0, -6.0, 2.0}, {0.0, 0.5, 0.0, -3.0}};
static double cubic(const double *a, double t) { return a[0] + t * (a[1] + t * (a[2] + t * a[3])); }
static double cubic_bound(const double *a, double t, double S) {
    const double T = std::fmax(1.0, std::fabs(t));
    const double A = std::fabs(a[0]) + T * (std::fabs(a[1]) + T * (std::fabs(a[2]) + T * std::fabs(a[3])));
    const double A1 = std::fabs(a[1]) + T * (2.0 * std::fabs(a[2]) + T * 3.0 * std::fabs(a[3]));
    return U * (19.0 * S * A + 6.0 * A + 3.5 * T * A1);
}

static int check(int nseg) {
    const int N = 3 * nseg + 1;
    double Lg[4];
    // the ends, exactly
    if (lagrange_segment(nseg, 0.0, Lg) != 0 || !is_unit(Lg, 0)) return fail("t = 0", nseg, Lg[0], Lg[1]);
    if (lagrange_segment(nseg, 1.0, Lg) != nseg - 1 || !is_unit(Lg, 3)) return fail("t = 1", nseg, Lg[3], Lg[2]);
    // an interior boundary belongs to the later segment, exactly where s / nseg is exact
    if ((nseg & (nseg - 1)) == 0)
        for (int s = 1; s < nseg; s++)
            if (lagrange_segment(nseg, (double)s / nseg, Lg) != s || !is_unit(Lg, 0)) return fail("interior boundary", nseg, s, Lg[0]);

    // the node times: what mpcmp_time_nodes tabulates, increasing from 0 to 1
    const double f[4] = {0.0, 0.25, 0.75, 1.0};
    std::vector<double> tau(N);
    for (int k = 0; k < N; k++) tau[k] = node_time(nseg, k);
    for (int s = 0; s < nseg; s++)
        for (int j = 0; j < 4; j++) if (tau[3 * s + j] != (s + f[j]) / nseg) return fail("node time", nseg, 3 * s + j, tau[3 * s + j]);
    if (tau[0] != 0.0 || tau[N - 1] != 1.0) return fail("first / last node time", nseg, tau[0], tau[N - 1]);
    for (int k = 1; k < N; k++) if (!(tau[k] > tau[k - 1])) return fail("node times do not increase", nseg, k, tau[k]);
    // interpolating the node times at a node gives the node's time
    for (int k = 0; k < N; k++) {
        const int s = lagrange_segment(nseg, tau[k], Lg);
        if (s < 0 || s >= nseg) return fail("segment of a node", nseg, k, s);
        const double back = interp_channel(tau.data(), 1, s, Lg), bound = (14.0 * abs_sum(Lg) + 4.0) * U;
        if (!(std::fabs(back - tau[k]) <= bound)) return fail("identity at a node", nseg, back - tau[k], bound);
    }

    // a plan whose channels are cubics: x [N][14] (positions 0 .. 6, velocities 7 .. 13), u [N][7]; channel c is cubic c % 4 scaled by 1 + c
    std::vector<double> X(14 * N), Uc(7 * N);
    auto coef = [](int c, double *a) { for (int i = 0; i < 4; i++) a[i] = (1 + c) * COEF[c % 4][i]; };
    for (int k = 0; k < N; k++)
        for (int c = 0; c < 21; c++) {
            double a[4];
            coef(c, a);
            (c < 14 ? X[14 * k + c] : Uc[7 * k + c - 14]) = cubic(a, tau[k]);
        }
    // off-node times inside, and outside [0, 1]: there the first / last segment is extrapolated
    std::vector<double> ts;
    for (int i = 0; i < 16 * nseg; i++) ts.push_back((i + 0.37) / (16 * nseg));
    const double outside[4] = {-0.1, -1e-9, 1.0 + 1e-9, 1.1};
    for (double t : outside) ts.push_back(t);
    for (double t : ts) {
        const int s = lagrange_segment(nseg, t, Lg);
        int want = (int)std::floor(t * nseg);
        want = want < 0 ? 0 : (want > nseg - 1 ? nseg - 1 : want);
        if (s != want) return fail("segment", nseg, t, s);
        if (t < 0.0 && s != 0) return fail("t < 0 does not clamp to segment 0", nseg, t, s);
        if (t > 1.0 && s != nseg - 1) return fail("t > 1 does not clamp to the last segment", nseg, t, s);
        const double S = abs_sum(Lg), sum = Lg[0] + Lg[1] + Lg[2] + Lg[3];
        if (!(std::fabs(sum - 1.0) <= 12.0 * U * S)) return fail("weights do not sum to 1", nseg, sum - 1.0, 12.0 * U * S);
        if (t < 0.0 && !(Lg[0] > 1.0)) return fail("t < 0 does not extrapolate", nseg, t, Lg[0]);
        if (t > 1.0 && !(Lg[3] > 1.0)) return fail("t > 1 does not extrapolate", nseg, t, Lg[3]);
        double q[7], v[7], ac[7], q2[7];
        interp_qva(X.data(), X.data() + 7, 14, Uc.data(), 7, s, Lg, q, v, ac);
        interp_q(X.data(), 14, s, Lg, q2);
        for (int r = 0; r < 7; r++) {
            // the three forms are one sum
            if (q[r] != interp_channel(X.data() + r, 14, s, Lg) || q2[r] != q[r] || v[r] != interp_channel(X.data() + 7 + r, 14, s, Lg) ||
                ac[r] != interp_channel(Uc.data() + r, 7, s, Lg)) return fail("the forms of the sum disagree", nseg, t, r);
            const double got[3] = {q[r], v[r], ac[r]};
            for (int g = 0; g < 3; g++) {
                double a[4];
                coef(7 * g + r, a);
                const double bound = cubic_bound(a, t, S);
                if (!(std::fabs(got[g] - cubic(a, t)) <= bound)) return fail("a cubic is not reproduced", nseg, got[g] - cubic(a, t), bound);
            }
        }
    }
    std::printf("ok %d\n", nseg);
    return 0;
}

int main() {
    const int nsegs[5] = {1, 2, 4, 6, 8};
    for (int nseg : nsegs) if (check(nseg)) return 1;
    return 0;
}
