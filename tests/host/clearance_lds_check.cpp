// Host-side check of the LDS layouts of the clearance kernels (mpc_motion_planner_amd/csrc/clearance_lds.hpp and the certified kernel's layout in
// clearance_cert.hpp), compiled and run by tests/test_clearance_lds_host.py under the address and undefined-behaviour sanitizers.  A layout is one
// function: a kernel carves its LDS with it and the launch asks for the bytes it counts.  For every table size the dynamic-LDS ceilings range over
// this program checks that the count equals the formula the kernels were launched with before the carves existed (copied below as the expected value:
// LDS per workgroup decides workgroups per CU, so it must not grow), and that the arrays of a carve lie inside that many bytes, do not overlap and are
// aligned to their element size; the first and last element of every array are written, so the sanitizer sees the bounds as well.
// Prints "ok <layouts>" or a diagnostic and exits non-zero.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../mpc_motion_planner_amd/csrc/clearance_cert.hpp"
#include "../../mpc_motion_planner_amd/csrc/clearance_lds.hpp"

using namespace mpcmp;

// ---- the formulas before the carves ----
static size_t old_bytes(size_t dbl, size_t ints) { return dbl * sizeof(double) + (ints + 1) / 2 * 2 * sizeof(int); }
static size_t old_clr(int narm, int N, int nsph, int n_obs, int chunk) {
    return old_bytes((size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 14 + (size_t)chunk * narm * 84 +
                         (size_t)chunk * nsph * 3,
                     (size_t)2 * nsph + (size_t)n_obs + (size_t)chunk);
}
static size_t old_mv(int narm, int N, int nsph, int n_obs, int chunk, int K) {
    return old_bytes((size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 14 + (size_t)chunk * narm * 84 +
                         (size_t)chunk * nsph * 3 + (size_t)3 * chunk + (size_t)3 * K,
                     (size_t)2 * nsph + (size_t)3 * n_obs + (size_t)3 * chunk);
}
static size_t old_fld(int narm, int N, int nsph, int chunk) {
    return old_bytes((size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)chunk * narm * 14 + (size_t)chunk * narm * 84, (size_t)nsph + (size_t)chunk);
}
static size_t old_cert(int narm, int N, int nsph, int n_obs, int chunk) {
    return old_bytes((size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)7 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 21 +
                         (size_t)chunk * narm * 84 + (size_t)chunk * nsph * 6,
                     (size_t)2 * CERT_CAP + (size_t)2 * nsph + (size_t)n_obs);
}
static size_t old_mvc(int narm, int N, int nsph, int n_obs, int n_tracks, int chunk) {
    return old_bytes((size_t)84 * narm + (size_t)7 * narm * N + (size_t)4 * nsph + (size_t)7 * nsph + (size_t)8 * n_obs + (size_t)chunk * narm * 21 +
                         (size_t)chunk * narm * 84 + (size_t)chunk * nsph * 6 + (size_t)chunk * n_tracks * 4,
                     (size_t)2 * CERT_CAP + (size_t)2 * nsph + (size_t)2 * n_obs);
}
static int old_chunk(int nsph, int per, int most) {
    const int c = nsph > 0 ? per / nsph : most;
    return c > most ? most : (c < 1 ? 1 : c);
}

// ---- one array of a carve: where it starts, its element size and its count ----
struct Arr { const char *name; char *p; size_t elem, n; };
static long n_layouts = 0;

static int check(const char *what, std::vector<Arr> arrs, char *base, size_t bytes, size_t expect, int narm, int nseg, int nsph, int n_obs, int x) {
    n_layouts++;
    if (bytes != expect) {
        std::printf("FAIL %s narm %d nseg %d nsph %d n_obs %d (%d): %zu bytes, expected %zu\n", what, narm, nseg, nsph, n_obs, x, bytes, expect);
        return 1;
    }
    std::sort(arrs.begin(), arrs.end(), [](const Arr &a, const Arr &b) { return a.p < b.p || (a.p == b.p && a.n < b.n); });
    char *end = base;
    for (const Arr &a : arrs) {
        if (a.n == 0) continue;
        if (a.p < end || a.p + a.elem * a.n > base + bytes || (uintptr_t)a.p % a.elem != 0) {
            std::printf("FAIL %s narm %d nseg %d nsph %d n_obs %d (%d): array %s at %td, %zu x %zu, after %td of %zu\n", what, narm, nseg, nsph, n_obs, x, a.name,
                        a.p - base, a.n, a.elem, end - base, bytes);
            return 1;
        }
        a.p[0] = 1; a.p[a.elem * a.n - 1] = 1;
        end = a.p + a.elem * a.n;
    }
    return 0;
}

#define A(L, m, count) Arr{#m, reinterpret_cast<char *>(L.m), sizeof(*L.m), (size_t)(count)}

static int sampled(int kind, const char *what, int narm, int nseg, int nsph, int n_obs, int K, size_t expect) {
    const ClrShape h = {narm, nseg, nsph < CLR_MAX_SPH ? nsph : CLR_MAX_SPH, nsph < CLR_MAX_SPH ? 0 : nsph - CLR_MAX_SPH, n_obs, 0, clr_chunk(nsph)};
    const size_t bytes = clr_lds_bytes(h, kind, K), N = 3 * nseg + 1, nq = 7 * narm, ch = h.chunk;
    const size_t tm = kind == CLR_LDS_TIMED, pr = kind != CLR_LDS_FIELD;
    char *base = static_cast<char *>(std::malloc(bytes ? bytes : 1));
    LdsCursor<true> c = {base, 0};
    const ClrLds L = clr_carve(c, h, kind, K);
    const int rc = check(what, {A(L, mk, 84 * narm), A(L, nodes, nq * N), A(L, sk, 4 * nsph), A(L, ok, 8 * n_obs), A(L, sc, ch * nq * 2), A(L, fr, ch * nq * 12),
                                A(L, cen, pr * ch * nsph * 3), A(L, ss, tm * ch), A(L, tt, tm * ch), A(L, pf, tm * ch), A(L, dly, tm * K), A(L, dk, tm * K),
                                A(L, w0, tm * K), A(L, sj, nsph), Arr{"sa", reinterpret_cast<char *>(L.sa), sizeof(int), pr * nsph}, A(L, ot, n_obs),
                                A(L, tof, tm * n_obs), A(L, lst, tm * n_obs), A(L, hit, ch), A(L, pk, tm * ch), A(L, pk1, tm * ch)},
                         base, bytes, expect, narm, nseg, nsph, n_obs, K);
    std::free(base);
    return rc || (kind == CLR_LDS_FIELD && L.sa != nullptr);
}

static int certified(bool timeline, int n_tracks, const char *what, int narm, int nseg, int nsph, int n_obs, size_t expect) {
    const CertShape h = {narm, nseg, nsph < CLR_MAX_SPH ? nsph : CLR_MAX_SPH, nsph < CLR_MAX_SPH ? 0 : nsph - CLR_MAX_SPH, n_obs, 0, cert_chunk(nsph), 1, 1, 0};
    const size_t bytes = cert_lds_bytes(h, timeline, n_tracks), N = 3 * nseg + 1, nq = 7 * narm, ch = h.chunk, nt = timeline ? n_tracks : 0;
    char *base = static_cast<char *>(std::malloc(bytes ? bytes : 1));
    const CertLds L = cert_layout(reinterpret_cast<double *>(base), h, timeline, n_tracks);
    const int rc = check(what, {A(L, mk, 84 * narm), A(L, nodes, nq * N), A(L, sk, 4 * nsph), A(L, rch, 7 * nsph), A(L, ok, 8 * n_obs), A(L, sc, ch * nq * 2),
                                A(L, dv, ch * nq), A(L, fr, ch * nq * 12), A(L, cen, ch * nsph * 3), A(L, Dl, ch * nsph), A(L, pd, ch * nsph), A(L, pl, ch * nsph),
                                A(L, tk, ch * nt * 4), A(L, cur, CERT_CAP), A(L, nxt, CERT_CAP), A(L, sj, nsph), A(L, sa, nsph), A(L, ot, n_obs),
                                A(L, tof, timeline ? n_obs : 0)},
                         base, bytes, expect, narm, nseg, nsph, n_obs, n_tracks);
    const bool end_ok = reinterpret_cast<char *>(L.end) <= base + bytes && reinterpret_cast<char *>(L.end) + 8 > base + bytes;
    std::free(base);
    if (!rc && !end_ok) std::printf("FAIL %s: the layout does not end at its byte count\n", what);
    return rc || !end_ok;
}

int main() {
    const int obs_counts[3] = {0, 1, CLR_MAX_OBS}, track_counts[3] = {0, 1, MPCMP_MAX_TRACKS}, delay_counts[2] = {0, MPCMP_MAX_DELAYS};
    for (int narm = 1; narm <= 2; narm++)
        for (int nseg = 1; nseg <= 8; nseg++)                // 4 to 25 nodes
            for (int nsph = 0; nsph <= narm * CLR_MAX_SPH; nsph++) {
                const int N = 3 * nseg + 1, chunk = clr_chunk(nsph), cchunk = cert_chunk(nsph);
                if (chunk != old_chunk(nsph, 1024, 32) || cchunk != old_chunk(nsph, 512, 16)) { std::printf("FAIL chunk of %d spheres\n", nsph); return 1; }
                if (sampled(CLR_LDS_FIELD, "k_clearance_field", narm, nseg, nsph, 0, 0, old_fld(narm, N, nsph, chunk))) return 1;
                for (int n_obs : obs_counts) {
                    if (sampled(CLR_LDS_SAMPLED, "k_clearance", narm, nseg, nsph, n_obs, 0, old_clr(narm, N, nsph, n_obs, chunk))) return 1;
                    for (int K : delay_counts)             // (K == 0: k_clearance_timed and, without obstacles, k_sphere_tracks; K > 0: k_start_delay)
                        if (sampled(CLR_LDS_TIMED, "moving.hip", narm, nseg, nsph, n_obs, K, old_mv(narm, N, nsph, n_obs, chunk, K))) return 1;
                    if (certified(false, 0, "k_clearance_cert", narm, nseg, nsph, n_obs, old_cert(narm, N, nsph, n_obs, cchunk))) return 1;
                    for (int nt : track_counts)
                        if (certified(true, nt, "k_clearance_cert_timed", narm, nseg, nsph, n_obs, old_mvc(narm, N, nsph, n_obs, nt, cchunk))) return 1;
                }
            }
    std::printf("ok %ld\n", n_layouts);
    return 0;
}
