// frame.hip — camera frames as voxel worlds (include/mpcmp_frame.h): the filter table k_frame_spheres, the classifying marker k_frame_mark over its
// three sources (a cloud, a depth image of 16-bit integers or of floats) and the carver k_frame_carve.  A translation unit of its own, so that
// k_field_mark, the transform and every check compile exactly as before.  The rule's arithmetic is frame_rule.hpp, the chain that of
// clearance_cert.hpp: the host statements of model_host.cpp run the same source.
#include <hip/hip_runtime.h>
#include <cmath>
#include "frame.hpp"

namespace mpcmp {

// One small launch per frame, one workgroup: the placements and the sines / cosines of both arms into LDS, one lane per arm runs the chain, then
// one lane per sphere writes (c_s, R_s^2).  The marker and the carver read the finished table, so no workgroup of theirs redoes the kinematics.
__global__ __launch_bounds__(FRM_MAX_SPH) void k_frame_spheres(const mpcmp_model *__restrict__ mdl, int narm, const ClrSphere *__restrict__ sph, int nsph,
                                                               FrmPosture q, double pad, double *__restrict__ tab) {
    __shared__ double mk[2 * 84], sc[2 * 14], fr[2 * 84];
    const int tid = threadIdx.x;
    for (int e = tid; e < 84 * narm; e += FRM_MAX_SPH) {
        const int a = e / 84, i = e % 84 / 12, c = e % 12;
        mk[e] = c < 9 ? mdl[a].R0[i][c] : mdl[a].p[i][c - 9];
    }
    if (tid < 7 * narm) {
        double sn, cs;
        sincos(q.q[tid], &sn, &cs);
        sc[2 * tid] = sn; sc[2 * tid + 1] = cs;
    }
    __syncthreads();
    if (tid < narm) cert_frames(mk + 84 * tid, sc + 14 * tid, fr + 84 * tid);
    __syncthreads();
    if (tid < nsph) {
        const ClrSphere s = sph[tid];
        double e[4];
        frm_entry(fr + 84 * s.arm + 12 * s.joint, s.c, s.r, pad, e);
        tab[4 * tid] = e[0]; tab[4 * tid + 1] = e[1]; tab[4 * tid + 2] = e[2]; tab[4 * tid + 3] = e[3];
    }
}

// the table into LDS once per workgroup; every lane then reads the same entry at the same time (a broadcast)
__device__ __forceinline__ void frm_stage(double *lt, const double *__restrict__ tab, int ns) {
    for (int e = threadIdx.x; e < 4 * ns; e += FRM_NT) lt[e] = tab[e];
    __syncthreads();
}
// one count of a class: the wave's lanes that hold `mine`, then ONE vector atomic per wave (by lane 0: every lane of a wave gets here)
__device__ __forceinline__ void frm_count(bool mine, int *counter) {
    const unsigned long long m = __ballot(mine);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(m));
}

// One lane per point or pixel: lane i reads item i, so the loads of a wave run over consecutive addresses (a depth image along its rows).  The
// class by frm_classify; a MARKED point stores 1 as a plain byte, as k_field_mark does.  Every lane of a workgroup stays to the end: the counts
// are ballots over whole waves.
template <int SRC>
__global__ __launch_bounds__(FRM_NT) void k_frame_mark(mpcmp_field_desc g, mpcmp_camera cam, int n, const void *__restrict__ src, const double *__restrict__ tab,
                                                       int ns, unsigned char *__restrict__ occ, mpcmp_frame_stats *__restrict__ stats) {
    __shared__ double lt[4 * FRM_MAX_SPH];
    frm_stage(lt, tab, ns);
    const int i = blockIdx.x * FRM_NT + threadIdx.x;
    const bool active = i < n;
    int code = -1 - FRM_INVALID;
    if (active) {
        double x[3];
        bool ok = true;
        if (SRC == FRM_SRC_POINTS) {
            const double *p = static_cast<const double *>(src) + 3 * (size_t)i;
            x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
        } else if (SRC == FRM_SRC_U16) {
            const unsigned short d = static_cast<const unsigned short *>(src)[i];
            ok = frm_pixel(cam, i % cam.width, i / cam.width, (double)d, frm_raw_ok_u16(d), x);
        } else {
            const float d = static_cast<const float *>(src)[i];
            ok = frm_pixel(cam, i % cam.width, i / cam.width, (double)d, frm_raw_ok_f32(d), x);
        }
        if (ok) code = frm_classify(g, lt, ns, x);
        if (code >= 0) occ[code] = 1;
    }
    const int cls = frm_class_of(code);
    frm_count(active, &stats->n_in);
    frm_count(active && cls == FRM_INVALID, &stats->n_invalid);
    frm_count(active && cls == FRM_OUTSIDE, &stats->n_outside);
    frm_count(active && cls == FRM_ROBOT, &stats->n_robot);
    frm_count(active && cls == FRM_MARKED, &stats->n_marked);
}

// Occupancy is sparse.  Lane i owns the four voxels 4 i .. 4 i + 3: it reads them as one dword, tests only the nonzero bytes against the table and
// writes its dword back only if it cleared one, so no two lanes touch the same byte.  The last lane of a grid whose voxel count is no multiple of
// four owns the nv % 4 bytes that are left and reads and writes them byte by byte.
__global__ __launch_bounds__(FRM_NT) void k_frame_carve(mpcmp_field_desc g, int nv, const double *__restrict__ tab, int ns, unsigned char *occ,
                                                        mpcmp_frame_stats *__restrict__ stats) {
    __shared__ double lt[4 * FRM_MAX_SPH];
    frm_stage(lt, tab, ns);
    const int i = blockIdx.x * FRM_NT + threadIdx.x, v0 = 4 * i;
    int cleared = 0;
    if (v0 + 4 <= nv) {
        unsigned w = reinterpret_cast<const unsigned *>(occ)[i];
        if (w != 0u) {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((w >> (8 * b)) & 0xFFu)
                    if (frm_carved(g, lt, ns, v0 + b)) { w &= ~(0xFFu << (8 * b)); cleared++; }
            if (cleared) reinterpret_cast<unsigned *>(occ)[i] = w;
        }
    } else if (v0 < nv) {
        for (int v = v0; v < nv; v++)
            if (occ[v] && frm_carved(g, lt, ns, v)) { occ[v] = 0; cleared++; }
    }
    // 0 <= cleared <= 4: its three bits, one ballot each
    const unsigned long long m0 = __ballot(cleared & 1), m1 = __ballot(cleared & 2), m2 = __ballot(cleared & 4);
    const int total = __popcll(m0) + 2 * __popcll(m1) + 4 * __popcll(m2);
    if (total != 0 && (threadIdx.x & 63) == 0) atomicAdd(&stats->n_cleared, total);
}

hipError_t frame_spheres_launch(const ClrTables &t, const FrmPosture &q, double pad, double *d_tab, hipStream_t st) {
    hipLaunchKernelGGL(k_frame_spheres, dim3(1), dim3(FRM_MAX_SPH), 0, st, t.d_model, t.narm, t.d_sph, t.n_sph[0] + t.n_sph[1], q, pad, d_tab);
    return hipGetLastError();
}

hipError_t frame_mark_launch(const FldArrays &f, int src, int n, const void *d_src, const mpcmp_camera *cam, const FrmFilter &flt, bool keep,
                             mpcmp_frame_stats *d_stats, hipStream_t st) {
    hipError_t e = hipMemsetAsync(d_stats, 0, sizeof(mpcmp_frame_stats), st);
    if (e == hipSuccess && !keep) e = hipMemsetAsync(f.d_occ, 0, (size_t)fld_voxels(f.desc), st);
    if (e != hipSuccess || n < 1) return e;
    const dim3 grid((n + FRM_NT - 1) / FRM_NT), block(FRM_NT);
    const mpcmp_camera c = cam ? *cam : mpcmp_camera{};
    if (src == FRM_SRC_POINTS) hipLaunchKernelGGL(k_frame_mark<FRM_SRC_POINTS>, grid, block, 0, st, f.desc, c, n, d_src, flt.d_tab, flt.ns, f.d_occ, d_stats);
    else if (src == FRM_SRC_U16) hipLaunchKernelGGL(k_frame_mark<FRM_SRC_U16>, grid, block, 0, st, f.desc, c, n, d_src, flt.d_tab, flt.ns, f.d_occ, d_stats);
    else hipLaunchKernelGGL(k_frame_mark<FRM_SRC_F32>, grid, block, 0, st, f.desc, c, n, d_src, flt.d_tab, flt.ns, f.d_occ, d_stats);
    return hipGetLastError();
}

hipError_t frame_carve_launch(const FldArrays &f, const FrmFilter &flt, mpcmp_frame_stats *d_stats, hipStream_t st) {
    hipError_t e = hipMemsetAsync(d_stats, 0, sizeof(mpcmp_frame_stats), st);
    if (e != hipSuccess || flt.ns < 1) return e;               // (no filter sphere: nothing can be cleared)
    const int nv = fld_voxels(f.desc), lanes = (nv + 3) / 4;
    hipLaunchKernelGGL(k_frame_carve, dim3((lanes + FRM_NT - 1) / FRM_NT), dim3(FRM_NT), 0, st, f.desc, nv, flt.d_tab, flt.ns, f.d_occ, d_stats);
    return hipGetLastError();
}

}  // namespace mpcmp
