// clearance.hip — batched clearance checks (include/mpcmp.h, "clearance"): robot spheres against obstacles and against the other arm, over the
// uniform samples of B trajectories; the choice of the fastest clear member of a group; and the host helpers that need no context.
// A translation unit of its own, so that the register-bound QP kernels of solver.hip compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "clearance_phases.hpp"

namespace mpcmp {

// One workgroup per trajectory.  Staged in LDS once: the joint placements of the arms, the node positions of the trajectory, the sphere tables and
// the problem's obstacles (in the form of clr_obs_prepare).  Then the n_pts + 1 samples in chunks of `chunk`, four phases per chunk:
//   A1  one thread per (sample, joint): the node interpolant of the joint position (plan_interp.hpp) and its sine / cosine;
//   A2  one thread per (sample, arm): the forward-kinematics chain, once per sample: world rotation and origin of the 7 joint frames
//       (A1 and A2 are clr_frames of clearance_phases.hpp, which the kernels of moving.hip and field.hip run as well);
//   B   one thread per (sample, sphere): world centre, then every obstacle (a uniform loop: all lanes read one obstacle, broadcast from LDS);
//   C   one thread per (sample, sphere s): every partner sphere t > s that clr_pair admits.
// Every thread keeps its best (clearance, packed index) pair in registers over all chunks; one workgroup reduction at the end orders them by
// clr_better, so the record does not depend on the launch or on the batch.  No atomics.  LDS use depends on the tables, not on n_pts.
__global__ __launch_bounds__(CLR_NT) void k_clearance(const mpcmp_model *__restrict__ mdl, int narm, int nseg, int n_pts,
                                                      const ClrSphere *__restrict__ sph, int n0, int n1,
                                                      const mpcmp_obstacle *__restrict__ obs, int n_obs, int obs_stride,
                                                      const double *__restrict__ sx, const double *__restrict__ sT, double margin, int self_gap,
                                                      int chunk_, mpcmp_clearance *__restrict__ out) {
    const ClrShape h = {narm, nseg, n0, n1, n_obs, obs_stride, chunk_};      // (scalar arguments: as one struct the kernel takes two registers more)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int nan_flag;
    const int b = blockIdx.x, tid = threadIdx.x, nsph = h.n0 + h.n1, chunk = h.chunk;
    LdsCursor<true> cur = {reinterpret_cast<char *>(lds), 0};
    const ClrLds L = clr_carve(cur, h, CLR_LDS_SAMPLED, 0);
    clr_stage(L, h, mdl, sph, obs, sx, b);               // (a NaN is flagged by the interpolated sample, below, not by the node)
    if (tid == 0) nan_flag = 0;
    __syncthreads();

    double best_d = INFINITY;
    unsigned best_k = CLR_NO_PAIR;
    int n_hit = 0, first = -1;                           // (thread 0 only)
    const bool pairs = h.narm > 1 || self_gap > 0;
    for (int ip0 = 0; ip0 <= n_pts; ip0 += chunk) {
        const int ns = (n_pts + 1 - ip0 < chunk) ? n_pts + 1 - ip0 : chunk;      // samples of this chunk
        // A1, A2
        clr_frames(L, h, ns, [&](int sl) { return (double)(ip0 + sl) / n_pts; }, &nan_flag);
        // B
        for (int it = tid; it < ns * nsph; it += CLR_NT) {
            const int sl = it / nsph, s = it % nsph;
            double c[3];
            clr_centre(L, h, sl, s, c);
            L.cen[3 * it] = c[0]; L.cen[3 * it + 1] = c[1]; L.cen[3 * it + 2] = c[2];
            double dm = INFINITY;
            int om = 0;
            for (int o = 0; o < h.n_obs; o++) {
                const double d = clr_sd(L.ot[o], L.ok + 8 * o, c[0], c[1], c[2]) - L.sk[4 * s + 3];
                if (d < dm) { dm = d; om = o; }
            }
            if (dm < margin) L.hit[sl] = 1;
            const unsigned k = clr_pack(ip0 + sl, s, 0, om);
            if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; }
        }
        __syncthreads();
        // C
        if (pairs) {
            for (int it = tid; it < ns * nsph; it += CLR_NT) {
                const int sl = it / nsph, s = it % nsph;
                int tm;
                const double dm = clr_pairs(L, nsph, sl, s, self_gap, &tm);
                if (dm < margin) L.hit[sl] = 1;
                const unsigned k = clr_pack(ip0 + sl, s, 1, tm);
                if (dm < INFINITY && clr_better(dm, k, best_d, best_k)) { best_d = dm; best_k = k; }
            }
            __syncthreads();
        }
        if (tid == 0) clr_count_hits(L, ns, ip0, &first, &n_hit);
    }
    clr_reduce(best_d, best_k, nullptr);
    if (tid == 0) out[b] = nan_flag ? clr_nan_record() : clr_record(best_d, best_k, first, n_hit, n_pts, sT[b]);
}

// ---- choice of the fastest admissible member of each group (mpcmp_select_clear_batch, mpcmp_select_checked_batch) ----
// clr and lim may each be null: that test is then skipped.  lim_bad = lim_mask | MPCMP_LIM_NAN
__device__ __forceinline__ bool sel_admissible(int i, const int *group, int n_groups, const mpcmp_info *info, const mpcmp_clearance *clr,
                                               const mpcmp_limits *lim, int lim_bad) {
    const int g = group[i];
    const int bad = MPCMP_STATUS_NAN | MPCMP_STATUS_NOT_PD | MPCMP_STATUS_XCH_DEAD | MPCMP_STATUS_OUTSIDE_TOL | MPCMP_STATUS_T_OUT_OF_BOX;
    return g >= 0 && g < n_groups && (info[i].status & bad) == 0 && (!clr || clr[i].status == 0) && (!lim || (lim[i].status & lim_bad) == 0);
}
// keys [n_groups] preset to all ones: the smallest ordered key of the admissible members' final times (an integer minimum: order-independent)
__global__ __launch_bounds__(256) void k_select_tmin(int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                                                     const mpcmp_limits *lim, int lim_bad, const int *group, int n_groups, unsigned long long *keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || !sel_admissible(i, group, n_groups, info, clr, lim, lim_bad)) return;
    atomicMin(keys + group[i], clr_tkey(sT[i]));
}
// chosen [n_groups] preset to 0x7F7F7F7F: the lowest index among the members that hold the group's key
__global__ __launch_bounds__(256) void k_select_index(int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                                                      const mpcmp_limits *lim, int lim_bad, const int *group, int n_groups,
                                                      const unsigned long long *keys, int *chosen) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B || !sel_admissible(i, group, n_groups, info, clr, lim, lim_bad)) return;
    if (clr_tkey(sT[i]) == keys[group[i]]) atomicMin(chosen + group[i], i);
}
__global__ __launch_bounds__(256) void k_select_finish(int n_groups, int *chosen) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_groups && chosen[g] == 0x7F7F7F7F) chosen[g] = -1;
}

hipError_t clearance_prepare() {
    // the largest tables need more than the 64 KB a kernel may use without asking: two arms, 25 nodes, 256 obstacles: 96 KB
    const size_t mx = lds_ceiling([](int s) { return clr_lds_bytes(ClrShape{2, 8, s, 0, CLR_MAX_OBS, 0, clr_chunk(s)}, CLR_LDS_SAMPLED, 0); });
    return hipFuncSetAttribute((const void *)k_clearance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mx);
}

hipError_t clearance_launch(const ClrTables &t, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                            mpcmp_clearance *d_out, hipStream_t st) {
    const ClrShape h = clr_shape(t, true);
    hipLaunchKernelGGL(k_clearance, dim3(B), dim3(CLR_NT), clr_lds_bytes(h, CLR_LDS_SAMPLED, 0), st, t.d_model, h.narm, h.nseg, n_pts, t.d_sph, h.n0, h.n1, t.d_obs,
                       h.n_obs, h.obs_stride, d_sx, d_sT, margin, self_gap, h.chunk, d_out);
    return hipGetLastError();
}

hipError_t select_launch(int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr, const mpcmp_limits *d_lim, int lim_mask,
                         const int *d_group, int n_groups, unsigned long long *d_keys, int *d_chosen, hipStream_t st) {
    const int lim_bad = lim_mask | MPCMP_LIM_NAN;
    if (n_groups < 1) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_keys, 0xFF, sizeof(unsigned long long) * n_groups, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_chosen, 0x7F, sizeof(int) * n_groups, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_tmin, dim3((B + 255) / 256), dim3(256), 0, st, B, d_sT, d_info, d_clr, d_lim, lim_bad, d_group, n_groups, d_keys);
    hipLaunchKernelGGL(k_select_index, dim3((B + 255) / 256), dim3(256), 0, st, B, d_sT, d_info, d_clr, d_lim, lim_bad, d_group,
                       n_groups, (const unsigned long long *)d_keys, d_chosen);
    hipLaunchKernelGGL(k_select_finish, dim3((n_groups + 255) / 256), dim3(256), 0, st, n_groups, d_chosen);
    return hipGetLastError();
}

}  // namespace mpcmp

using namespace mpcmp;

// ---- host helpers (no GPU) ----
extern "C" int mpcmp_link_spheres(const mpcmp_model *model, double radius, double spacing, int max, mpcmp_sphere *out, int *n) {
    if (!model || !out || !n || !(radius > 0.0) || !(spacing > 0.0) || !std::isfinite(radius) || !std::isfinite(spacing) || max < 0) return MPCMP_EINVAL;
    int cnt = 0;
    for (int pass = 0; pass < 2; pass++) {          // count first: nothing is written when the spheres do not fit
        cnt = 0;
        for (int i = 0; i < 7; i++) {
            const double *e = i < 6 ? model->p[i + 1] : model->tool;
            const double L = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            const int k = L > 0.0 ? (int)std::ceil(L / spacing) + 1 : 1;
            for (int c = 0; c < k; c++, cnt++) {
                if (!pass) continue;
                const double f = k > 1 ? (double)c / (k - 1) : 0.0;
                mpcmp_sphere &s = out[cnt];
                s.joint = i; s.pad = 0; s.r = radius;
                for (int d = 0; d < 3; d++) s.c[d] = f * e[d];
            }
        }
        if (cnt > max) return MPCMP_EINVAL;
    }
    *n = cnt;
    return MPCMP_OK;
}

// World placement of every joint frame: p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i).  Not cert_frames: this statement adds the
// three products to p_w one after the other, cert_frames (and every kernel) adds their sum, and the last bits of mpcmp_clearance_config are public
static void fk_frames(const mpcmp_model *m, const double *q, double Rw[7][9], double pw[7][3]) {
    double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, pp[3] = {0, 0, 0};
    for (int i = 0; i < 7; i++) {
        const double s = std::sin(q[i]), c = std::cos(q[i]), *A = m->R0[i];
        double R[9];
        for (int r = 0; r < 3; r++) { R[3 * r] = A[3 * r] * c + A[3 * r + 1] * s; R[3 * r + 1] = -A[3 * r] * s + A[3 * r + 1] * c; R[3 * r + 2] = A[3 * r + 2]; }
        for (int r = 0; r < 3; r++) pw[i][r] = pp[r] + Rp[3 * r] * m->p[i][0] + Rp[3 * r + 1] * m->p[i][1] + Rp[3 * r + 2] * m->p[i][2];
        for (int r = 0; r < 3; r++)
            for (int c2 = 0; c2 < 3; c2++) Rw[i][3 * r + c2] = Rp[3 * r] * R[c2] + Rp[3 * r + 1] * R[3 + c2] + Rp[3 * r + 2] * R[6 + c2];
        std::memcpy(Rp, Rw[i], sizeof Rp); std::memcpy(pp, pw[i], sizeof pp);
    }
}

extern "C" int mpcmp_clearance_config(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                      const mpcmp_obstacle *obs, int self_gap, const double *q, double *d_min, int *sphere, int *other) {
    if (!models || narm < 1 || narm > 2 || !n_spheres || !q || !d_min || n_obs < 0 || n_obs > CLR_MAX_OBS || (n_obs > 0 && !obs) || self_gap < 0)
        return MPCMP_EINVAL;
    int nsph = 0;
    for (int a = 0; a < narm; a++) { if (n_spheres[a] < 0 || n_spheres[a] > CLR_MAX_SPH) return MPCMP_EINVAL; nsph += n_spheres[a]; }
    if (nsph > 0 && !spheres) return MPCMP_EINVAL;
    double cen[2 * CLR_MAX_SPH][3], rad[2 * CLR_MAX_SPH];
    int arm[2 * CLR_MAX_SPH], jnt[2 * CLR_MAX_SPH];
    for (int a = 0, s = 0; a < narm; a++) {
        double Rw[7][9], pw[7][3];
        fk_frames(models + a, q + 7 * a, Rw, pw);
        for (int k = 0; k < n_spheres[a]; k++, s++) {
            const mpcmp_sphere &S = spheres[s];
            if (S.joint < 0 || S.joint > 6) return MPCMP_EINVAL;
            const double *R = Rw[S.joint];
            for (int r = 0; r < 3; r++) cen[s][r] = pw[S.joint][r] + R[3 * r] * S.c[0] + R[3 * r + 1] * S.c[1] + R[3 * r + 2] * S.c[2];
            rad[s] = S.r; arm[s] = a; jnt[s] = S.joint;
        }
    }
    double best = INFINITY;
    unsigned bk = CLR_NO_PAIR;
    for (int s = 0; s < nsph; s++) {
        for (int o = 0; o < n_obs; o++) {
            double k[8];
            clr_obs_prepare(obs[o], k);
            const double d = clr_sd(obs[o].type, k, cen[s][0], cen[s][1], cen[s][2]) - rad[s];
            const unsigned key = clr_pack(0, s, 0, o);
            if (clr_better(d, key, best, bk)) { best = d; bk = key; }
        }
        for (int t = s + 1; t < nsph; t++) {
            if (!clr_pair(arm[s], jnt[s], arm[t], jnt[t], self_gap)) continue;
            const double ex = cen[s][0] - cen[t][0], ey = cen[s][1] - cen[t][1], ez = cen[s][2] - cen[t][2];
            const double d = std::sqrt(ex * ex + ey * ey + ez * ez) - rad[s] - rad[t];
            const unsigned key = clr_pack(0, s, 1, t);
            if (clr_better(d, key, best, bk)) { best = d; bk = key; }
        }
    }
    int sp = -1, ot = 0;
    if (bk != CLR_NO_PAIR) clr_unpack(bk, &sp, &ot);
    *d_min = best;
    if (sphere) *sphere = sp;
    if (other) *other = ot;
    return MPCMP_OK;
}
