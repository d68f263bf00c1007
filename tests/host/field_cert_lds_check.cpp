// Host-side check of what mpc_motion_planner_amd/csrc/field_cert_rule.hpp states once for the kernel and its launch, compiled and run by
// tests/test_field_cert_host.py under the address and undefined-behaviour sanitizers:
//   - the LDS layout of k_clearance_cert_field (MPCMP_FCERT_LAYOUT): for every table size the dynamic-LDS ceiling ranges over, the byte count equals
//     the sum of the arrays written out below, stays under the 160 KB of a CU, and the arrays lie inside that many bytes, do not overlap and are
//     aligned to their element size; the first and last element of every array are written, so the sanitizer sees the bounds as well;
//   - the chunk: between 1 and 64 (one deciding lane of the first wave per interval), and the chunk's arrays within their budget;
//   - the row pitch of pd and pl: odd and at least the chunk;
//   - the certificate merge fcert_merge: the smaller bound with its time, ties to a, +inf, sums, the larger depth, and NaN.
// Prints "ok <layouts>" or a diagnostic and exits non-zero.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../mpc_motion_planner_amd/csrc/field_cert_rule.hpp"

using namespace mpcmp;

struct Arr { const char *name; char *p; size_t elem, n; };
#define A(L, m, count) Arr{#m, reinterpret_cast<char *>(L.m), sizeof(*L.m), (size_t)(count)}

static int layout(int narm, int nseg, int nsph) {
    const int chunk = fcert_chunk(narm, nsph), pitch = fcert_pitch(chunk);
    if (chunk < 1 || chunk > 64 || chunk > FCERT_CHUNK_MAX || pitch < chunk || pitch % 2 != 1 || pitch > chunk + 1) {
        std::printf("FAIL chunk %d pitch %d of %d arms, %d spheres\n", chunk, pitch, narm, nsph);
        return 1;
    }
    if (chunk > 1 && (size_t)chunk * (105 * narm + 2 * nsph) > (size_t)FCERT_CHUNK_DOUBLES) {
        std::printf("FAIL chunk %d of %d arms, %d spheres exceeds its budget\n", chunk, narm, nsph);
        return 1;
    }
    const FcertShape h = {narm, nseg, nsph < CLR_MAX_SPH ? nsph : CLR_MAX_SPH, nsph < CLR_MAX_SPH ? 0 : nsph - CLR_MAX_SPH, chunk, 1, 0};
    const size_t bytes = fcert_lds_bytes(h), N = 3 * nseg + 1, nq = 7 * narm, ch = chunk;
    const size_t dbl = 84 * narm + nq * N + 11 * (size_t)nsph + ch * nq * 15 + 2 * (size_t)nsph * pitch, ints = 2 * (size_t)CERT_CAP + 2 * (size_t)nsph;
    const size_t expect = dbl * sizeof(double) + (ints + 1) / 2 * 2 * sizeof(int);
    if (bytes != expect || bytes > 160 * 1024) {
        std::printf("FAIL narm %d nseg %d nsph %d: %zu bytes, expected %zu (at most 163840)\n", narm, nseg, nsph, bytes, expect);
        return 1;
    }
    char *base = static_cast<char *>(std::malloc(bytes));
    const FcertLds L = fcert_layout(reinterpret_cast<double *>(base), h);
    std::vector<Arr> arrs = {A(L, mk, 84 * narm), A(L, nodes, nq * N), A(L, sk, 4 * nsph), A(L, rch, 7 * nsph), A(L, sc, ch * nq * 2), A(L, dv, ch * nq),
                             A(L, fr, ch * nq * 12), A(L, pd, (size_t)nsph * pitch), A(L, pl, (size_t)nsph * pitch), A(L, cur, CERT_CAP), A(L, nxt, CERT_CAP),
                             A(L, sj, nsph), A(L, sa, nsph)};
    std::sort(arrs.begin(), arrs.end(), [](const Arr &a, const Arr &b) { return a.p < b.p || (a.p == b.p && a.n < b.n); });
    char *end = base;
    int rc = 0;
    for (const Arr &a : arrs) {
        if (a.n == 0) continue;
        if (a.p < end || a.p + a.elem * a.n > base + bytes || (uintptr_t)a.p % a.elem != 0) {
            std::printf("FAIL narm %d nseg %d nsph %d: array %s at %td, %zu x %zu, after %td of %zu\n", narm, nseg, nsph, a.name, a.p - base, a.n, a.elem,
                        end - base, bytes);
            rc = 1;
            break;
        }
        a.p[0] = 1; a.p[a.elem * a.n - 1] = 1;
        end = a.p + a.elem * a.n;
    }
    if (!rc && !(reinterpret_cast<char *>(L.end) <= base + bytes && reinterpret_cast<char *>(L.end) + 8 > base + bytes)) {
        std::printf("FAIL narm %d nseg %d nsph %d: the layout does not end at its byte count\n", narm, nseg, nsph);
        rc = 1;
    }
    std::free(base);
    return rc;
}

static mpcmp_clearance_cert cert(double d, double t, int e, int c, int u, int depth) {
    mpcmp_clearance_cert r;
    r.d_lower = d; r.t_lower = t; r.n_eval = e; r.n_clear = c; r.n_undecided = u; r.depth = depth;
    return r;
}
static bool same(const mpcmp_clearance_cert &g, double d, double t, int e, int c, int u, int depth) {
    const bool dd = std::isnan(d) ? std::isnan(g.d_lower) : g.d_lower == d;
    return dd && g.t_lower == t && g.n_eval == e && g.n_clear == c && g.n_undecided == u && g.depth == depth;
}
static int merge() {
    const double inf = INFINITY;
    const mpcmp_clearance_cert a = cert(0.25, 1.5, 20, 17, 1, 3), b = cert(0.125, 0.5, 16, 16, 0, 0), tie = cert(0.25, 0.75, 4, 4, 0, 7),
                               none = cert(inf, 0.0625, 16, 16, 0, 0), none2 = cert(inf, 0.125, 8, 8, 0, 0), nan = cert_nan_record();
    if (!same(fcert_merge(a, b), 0.125, 0.5, 36, 33, 1, 3) || !same(fcert_merge(b, a), 0.125, 0.5, 36, 33, 1, 3)) return 1;
    if (!same(fcert_merge(a, tie), 0.25, 1.5, 24, 21, 1, 7) || !same(fcert_merge(tie, a), 0.25, 0.75, 24, 21, 1, 7)) return 2;      // ties to a
    if (!same(fcert_merge(a, none), 0.25, 1.5, 36, 33, 1, 3) || !same(fcert_merge(none, a), 0.25, 1.5, 36, 33, 1, 3)) return 3;
    if (!same(fcert_merge(none, none2), inf, 0.0625, 24, 24, 0, 0) || !same(fcert_merge(none2, none), inf, 0.125, 24, 24, 0, 0)) return 4;
    if (!same(fcert_merge(a, nan), NAN, -1.0, 0, 0, 0, 0) || !same(fcert_merge(nan, a), NAN, -1.0, 0, 0, 0, 0) ||
        !same(fcert_merge(nan, nan), NAN, -1.0, 0, 0, 0, 0)) return 5;
    if (fcert_key(5u, 3) != cert_key(5u, 3, 0, 0) || !(fcert_key(5u, 3) < fcert_key(5u, 4)) || !(fcert_key(5u, 63) < fcert_key(6u, 0))) return 6;
    return 0;
}

int main() {
    long n = 0;
    for (int narm = 1; narm <= 2; narm++)
        for (int nseg = 1; nseg <= 8; nseg++)                // 4 to 25 nodes
            for (int nsph = 0; nsph <= narm * CLR_MAX_SPH; nsph++, n++)
                if (layout(narm, nseg, nsph)) return 1;
    if (int rc = merge()) { std::printf("FAIL merge %d\n", rc); return 1; }
    std::printf("ok %ld\n", n);
    return 0;
}
