// field.hip — voxel worlds (include/mpcmp_field.h): the point marker k_field_mark, the exact squared distance transform in three separable passes
// (k_field_pass_x, then k_field_pass along y and along z), the field check k_clearance_field and the record merge k_clearance_merge.  A translation
// unit of its own, so that k_clearance and every other kernel compile exactly as before.  The rule's arithmetic is field_rule.hpp, the frames and
// centres those of clearance_cert.hpp, the tie order that of clearance_rule.hpp: the host statements of model_host.cpp run the same source.
#include <hip/hip_runtime.h>
#include <cmath>
#include "field.hpp"
#include "clearance_phases.hpp"

namespace mpcmp {

// one lane per point: a plain byte store of 1 (identical concurrent stores are harmless; no atomics)
__global__ __launch_bounds__(256) void k_field_mark(mpcmp_field_desc g, int n_points, const double *__restrict__ pts, unsigned char *__restrict__ occ) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    const int v = fld_point_voxel(g, p);
    if (v >= 0) occ[v] = 1;
}

// The transform is the O(n^2) min-plus sweep per line (fld_step): exact, branch-free, integers only, no atomics.
//
// Pass x.  Lines along x are contiguous in memory, and so are neighbouring lines: a workgroup stages `lpb` whole lines (at most 1024 entries, each
// line padded with FLD_INF to a multiple of four entries so that a lane reads four of them at once), one lane per output.  Lanes of one line read
// the same LDS address (a broadcast); loads and stores of global memory run over consecutive addresses.
constexpr int FLD_XTILE = 1024;      // lpb lines of pitch P <= 1024: lpb = max(1, 1024 / P) (field_build_launch), so lpb P <= 1024
__global__ __launch_bounds__(FLD_NT) void k_field_pass_x(const unsigned char *__restrict__ occ, unsigned *__restrict__ out, int n0, int n_lines, int lpb) {
    __shared__ __attribute__((aligned(16))) unsigned g[FLD_XTILE];
    const int tid = threadIdx.x, P = (n0 + 3) & ~3, line0 = blockIdx.x * lpb;
    const int nl = n_lines - line0 < lpb ? n_lines - line0 : lpb;
    for (int e = tid; e < nl * P; e += FLD_NT) {
        const int l = e / P, i = e % P;
        g[e] = (i < n0 && occ[(size_t)(line0 + l) * n0 + i]) ? 0u : FLD_INF;
    }
    __syncthreads();
    for (int e = tid; e < nl * n0; e += FLD_NT) {
        const int l = e / n0, i = e % n0;
        const uint4 *L = reinterpret_cast<const uint4 *>(g + l * P);
        unsigned best = FLD_INF;
        for (int k = 0; k < P; k += 4) {
            const uint4 v = L[k >> 2];
            best = fld_step(best, v.x, i - k);
            best = fld_step(best, v.y, i - k - 1);
            best = fld_step(best, v.z, i - k - 2);
            best = fld_step(best, v.w, i - k - 3);
        }
        out[(size_t)line0 * n0 + e] = best;
    }
}

// Passes y and z.  A line runs along an axis whose neighbours in memory are `line_stride` entries apart; the `nx` columns beside it are contiguous
// (pass y: the n0 entries of a row, once per z plane = `outer`; pass z: the n0 n1 entries of a plane).  A workgroup takes a tile of TX = 2^txl
// neighbouring columns by the WHOLE line into LDS (n TX <= FLD_TILE entries): adjacent lanes read and write adjacent columns, in global memory and
// in LDS alike, and no lane-to-lane stride is a line length.  Lane (tx, ty) owns four outputs of column tx per round, rows ty + r 256 / TX, so that
// one LDS read serves four steps.  `final`: the last pass writes MPCMP_FIELD_EMPTY for FLD_INF.
__global__ __launch_bounds__(FLD_NT) void k_field_pass(const unsigned *__restrict__ in, unsigned *__restrict__ out, int nx, int n, int line_stride,
                                                       int outer_stride, int txl, int tiles, int final) {
    extern __shared__ __attribute__((aligned(16))) unsigned gt[];
    const int tid = threadIdx.x, TX = 1 << txl, rows = FLD_NT >> txl;
    const int tile = blockIdx.x % tiles, outer = blockIdx.x / tiles;
    const int tx = tid & (TX - 1), ty = tid >> txl, x = tile * TX + tx;
    const bool valid = x < nx;
    const size_t base = (size_t)outer * outer_stride + x;
    for (int j = ty; j < n; j += rows) gt[(j << txl) + tx] = valid ? in[base + (size_t)j * line_stride] : FLD_INF;
    __syncthreads();
    for (int j0 = ty; j0 < n; j0 += 4 * rows) {
        unsigned b0 = FLD_INF, b1 = FLD_INF, b2 = FLD_INF, b3 = FLD_INF;
        for (int k = 0; k < n; k++) {
            const unsigned v = gt[(k << txl) + tx];
            const int d = j0 - k;
            b0 = fld_step(b0, v, d);
            b1 = fld_step(b1, v, d + rows);
            b2 = fld_step(b2, v, d + 2 * rows);
            b3 = fld_step(b3, v, d + 3 * rows);
        }
        const unsigned b[4] = {b0, b1, b2, b3};
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = j0 + r * rows;
            if (valid && j < n) out[base + (size_t)j * line_stride] = (final && b[r] >= FLD_INF) ? MPCMP_FIELD_EMPTY : b[r];
        }
    }
}

// One workgroup per plan, the shape of k_clearance: the tables staged in LDS once, then the samples in chunks of `chunk`, and per chunk
//   A1  one thread per (sample, joint): the node interpolant of the joint position and its sine / cosine;
//   A2  one thread per (sample, arm): the forward-kinematics chain;
//   B   one thread per (sample, sphere): world centre, one entry of the field, sqrt in double.
// The field stays in global memory: one dword gather per (sample, sphere).  The voxel read is carried beside the (value, key) pair.
__global__ __launch_bounds__(CLR_NT) void k_clearance_field(const mpcmp_model *__restrict__ mdl, ClrShape h, int n_pts, const ClrSphere *__restrict__ sph,
                                                            mpcmp_field_desc g, const unsigned *__restrict__ d2, const double *__restrict__ sx,
                                                            const double *__restrict__ sT, double margin, mpcmp_clearance *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    LdsCursor<true> cur = {reinterpret_cast<char *>(lds), 0};
    const ClrLds L = clr_carve(cur, h, CLR_LDS_FIELD, 0);
    clr_stage(L, h, mdl, sph, nullptr, sx, b);               // (h.n_obs == 0: no obstacle is read; a NaN is flagged by the interpolated sample)
    if (tid == 0) nan_flag = 0;
    __syncthreads();

    double best_d = INFINITY;
    unsigned best_k = CLR_NO_PAIR;
    int best_v = 0;
    int n_hit = 0, first = -1;                               // (thread 0 only)
    for (int ip0 = 0; ip0 <= n_pts; ip0 += chunk) {
        const int ns = (n_pts + 1 - ip0 < chunk) ? n_pts + 1 - ip0 : chunk;
        // A1, A2
        clr_frames(L, h, ns, [&](int sl) { return (double)(ip0 + sl) / n_pts; }, &nan_flag);
        // B.  A NaN plan's centres are not looked up (its record is the NaN record whatever is found here); fld_sd clamps every finite centre onto
        // the grid, so the gather stays inside the field
        if (!nan_flag)
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                double c[3];
                clr_centre(L, h, sl, s, c);
                int v = 0;
                double dm = INFINITY;
                if (fld_finite(c[0]) && fld_finite(c[1]) && fld_finite(c[2])) dm = fld_sd(g, d2, c[0], c[1], c[2], &v) - L.sk[4 * s + 3];
                if (dm < margin) L.hit[sl] = 1;
                const unsigned k = clr_pack(ip0 + sl, s, 0, 0);
                if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; best_v = v; }
            }
        __syncthreads();
        if (tid == 0) clr_count_hits(L, ns, ip0, &first, &n_hit);
    }
    clr_reduce(best_d, best_k, &best_v);                     // (the voxel carried beside the key)
    if (tid == 0) {
        mpcmp_clearance r = nan_flag ? clr_nan_record() : clr_record(best_d, best_k, first, n_hit, n_pts, sT[b]);
        if (!nan_flag && best_k != CLR_NO_PAIR) r.other = best_v;
        out[b] = r;
    }
}

// one lane per problem
__global__ __launch_bounds__(256) void k_clearance_merge(int B, const mpcmp_clearance *a, const mpcmp_clearance *b, mpcmp_clearance *out, int *source) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    int src;
    const mpcmp_clearance r = fld_merge(a[i], b[i], &src);      // (both read before the write: out may be a or b)
    out[i] = r;
    if (source) source[i] = src;
}

hipError_t field_prepare() {
    // as clearance_prepare: two arms, 25 nodes
    const size_t mx = lds_ceiling([](int s) { return clr_lds_bytes(ClrShape{2, 8, s, 0, 0, 0, clr_chunk(s)}, CLR_LDS_FIELD, 0); });
    return hipFuncSetAttribute((const void *)k_clearance_field, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mx);
}

hipError_t field_mark_launch(const FldArrays &f, int n_points, const double *d_points, hipStream_t st) {
    hipError_t e = hipMemsetAsync(f.d_occ, 0, (size_t)fld_voxels(f.desc), st);
    if (e != hipSuccess || n_points < 1) return e;
    hipLaunchKernelGGL(k_field_mark, dim3((n_points + 255) / 256), dim3(256), 0, st, f.desc, n_points, d_points, f.d_occ);
    return hipGetLastError();
}

// the tile of a pass along a line of n entries beside nx contiguous columns: log2 of its width
static int fld_tile_log2(int n, int nx) {
    int l = 6;                                               // at most 64 columns
    while (l > 0 && ((n << l) > FLD_TILE || (1 << (l - 1)) >= nx)) l--;
    return l;
}

static hipError_t fld_pass_launch(const unsigned *in, unsigned *out, int nx, int n, int line_stride, int n_outer, int outer_stride, int final,
                                  hipStream_t st) {
    const int txl = fld_tile_log2(n, nx), tiles = (nx + (1 << txl) - 1) >> txl;
    hipLaunchKernelGGL(k_field_pass, dim3(tiles * n_outer), dim3(FLD_NT), sizeof(unsigned) * ((size_t)n << txl), st, in, out, nx, n, line_stride,
                       outer_stride, txl, tiles, final);
    return hipGetLastError();
}

hipError_t field_build_launch(const FldArrays &f, hipStream_t st) {
    const int n0 = f.desc.n[0], n1 = f.desc.n[1], n2 = f.desc.n[2], P = (n0 + 3) & ~3;
    const int n_lines = n1 * n2, lpb = 1024 / P > 256 ? 256 : (1024 / P < 1 ? 1 : 1024 / P);
    hipLaunchKernelGGL(k_field_pass_x, dim3((n_lines + lpb - 1) / lpb), dim3(FLD_NT), 0, st, f.d_occ, f.d_d2, n0, n_lines, lpb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = fld_pass_launch(f.d_d2, f.d_tmp, n0, n1, n0, n2, n0 * n1, 0, st);
    if (e != hipSuccess) return e;
    return fld_pass_launch(f.d_tmp, f.d_d2, n0 * n1, n2, n0 * n1, 1, 0, 1, st);
}

hipError_t clearance_field_launch(const ClrTables &t, const FldArrays &f, int B, const double *d_sx, const double *d_sT, int n_pts, double margin,
                                  mpcmp_clearance *d_out, hipStream_t st) {
    const ClrShape h = clr_shape(t, false);
    const size_t lds = clr_lds_bytes(h, CLR_LDS_FIELD, 0);
    hipLaunchKernelGGL(k_clearance_field, dim3(B), dim3(CLR_NT), lds, st, t.d_model, h, n_pts, t.d_sph, f.desc, f.d_d2, d_sx, d_sT, margin, d_out);
    return hipGetLastError();
}

hipError_t clearance_merge_launch(int B, const mpcmp_clearance *d_a, const mpcmp_clearance *d_b, mpcmp_clearance *d_out, int *d_source, hipStream_t st) {
    hipLaunchKernelGGL(k_clearance_merge, dim3((B + 255) / 256), dim3(256), 0, st, B, d_a, d_b, d_out, d_source);
    return hipGetLastError();
}

}  // namespace mpcmp
