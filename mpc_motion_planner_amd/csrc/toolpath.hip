// toolpath.hip — tool-line moves (include/mpcmp_toolpath.h): the generator that writes a straight tool path as a finished plan and the checker of
// its interpolant, both running the rule of toolpath.hpp.  A translation unit of its own, so that the register-bound QP kernels of solver.hip
// compile exactly as before.
#include <hip/hip_runtime.h>
#include <cmath>
#include "toolpath.hpp"

namespace mpcmp_tl {

// One lane per line: the continuation is serial along sigma.  The model is read through a wave-uniform address (one model for the batch), the
// problem's inputs are loaded into registers once, and tl_track writes the arm's columns of the plan node by node.  A lane that stops writes its
// NaN rows and leaves; no barriers, no atomics; LDS holds each lane's own TlWork slot and nothing shared.  Blocks of TL_NT = 32 lanes: the work per
// lane is long and latency-bound, so a batch of a few hundred lines is better spread over many CUs than packed into full blocks on two of them.
__global__ __launch_bounds__(TL_NT, 2) void k_tool_line(const mpcmp_model *__restrict__ mdl, int nseg, int B, const mpcmp_bounds *__restrict__ rows,
                                                        TlQRows table, int nx, int nu, int col_q, int col_v, int col_u,
                                                        const double *__restrict__ qs, const double *__restrict__ R1s, const double *__restrict__ p1s,
                                                        const double *Tin, mpcmp_tool_line_spec sp, double *sx, double *su, double *sT,
                                                        mpcmp_tool_line *__restrict__ out) {
    __shared__ TlWork work[TL_NT];
    const int b = blockIdx.x * TL_NT + threadIdx.x;
    if (b >= B) return;
    const int N = 3 * nseg + 1;
    double q0[7], R1[9], p1[3];
#pragma unroll
    for (int k = 0; k < 7; k++) q0[k] = qs[7 * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < 9; k++) R1[k] = R1s[9 * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < 3; k++) p1[k] = p1s[3 * (size_t)b + k];
    const double T_in = Tin ? Tin[b] : 0.0;
    mpcmp_tool_line rec;
    tl_track(*mdl, nseg, sp, q0, R1, p1, T_in, sx, nx, col_q, col_v, su, nu, col_u, b, &rec, work[threadIdx.x]);
    sT[b] = work[threadIdx.x].T;
    // the position rows are loaded only now: fourteen more values would live in registers through the whole continuation
    double lbq[7], ubq[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { lbq[k] = rows ? rows[b].lbx[k] : table.lb[k]; ubq[k] = rows ? rows[b].ubx[k] : table.ub[k]; }
    tl_q_excess(sx + (size_t)b * N * nx + col_q, nx, nseg, lbq, ubq, &rec);
    if (out) out[b] = rec;
}

// One workgroup of one wave per plan.  Staged in LDS once: the position nodes of the arm (at most 25 x 7 doubles) and the line, which lane 0 forms
// from the tool pose of node 0.  Then one thread per sample, in chunks of TD_NT samples, each keeping its TlDevAcc in registers; one wave reduction
// at the end combines them by tl_dev_merge (the larger value, of equal ones the lower sample index: exact, so the order of the butterfly does not
// matter).  No atomics, and LDS does not grow with n_pts.
__global__ __launch_bounds__(TD_NT, 2) void k_tool_deviation(const mpcmp_model *__restrict__ mdl, int nseg, int nx, int col_q, const double *__restrict__ sx,
                                                          const double *__restrict__ R1s, const double *__restrict__ p1s, int n_pts, double tol_lin,
                                                          double tol_ang, mpcmp_tool_dev *__restrict__ out) {
    __shared__ double Qs[TL_MAX_NODES * 7];
    __shared__ TlLine line;
    const int b = blockIdx.x, lane = threadIdx.x, N = 3 * nseg + 1;
    const double *X = sx + (size_t)b * N * nx + col_q;
    for (int e = lane; e < 7 * N; e += TD_NT) Qs[e] = X[(size_t)(e / 7) * nx + e % 7];
    __syncthreads();
    if (lane == 0) {
        double R1[9], p1[3];
#pragma unroll
        for (int k = 0; k < 9; k++) R1[k] = R1s[9 * (size_t)b + k];
#pragma unroll
        for (int k = 0; k < 3; k++) p1[k] = p1s[3 * (size_t)b + k];
        TlLine Ln;
        tl_line_of_plan(*mdl, Qs, R1, p1, Ln);
        line = Ln;
    }
    __syncthreads();
    const TlLine Ln = line;
    TlDevAcc A;
    tl_dev_init(A);
#pragma nounroll
    for (int i = lane; i <= n_pts; i += TD_NT) {
        double dl, dp, da;
        tl_dev_sample(*mdl, Ln, nseg, Qs, 7, i, n_pts, &dl, &dp, &da);
        tl_dev_fold(A, i, dl, dp, da, tol_lin, tol_ang);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ol = __shfl_xor(A.lin, off), op = __shfl_xor(A.perp, off), oa = __shfl_xor(A.ang, off);
        const int il = __shfl_xor(A.i_lin, off), ia = __shfl_xor(A.i_ang, off), no = __shfl_xor(A.n_over, off), nn = __shfl_xor(A.nan, off);
        tl_dev_merge(A, ol, il, op, oa, ia, no, nn);
    }
    if (lane == 0) out[b] = tl_dev_record(A, n_pts);
}

hipError_t tool_line_launch(const mpcmp_model *mdl, int nseg, int B, const mpcmp_bounds *rows, const mpcmp_bounds &table, int nx, int nu, int col_q,
                            int col_v, int col_u, const double *d_q, const double *d_R1, const double *d_p1, const double *d_Tin,
                            const mpcmp_tool_line_spec &spec, double *d_sx, double *d_su, double *d_sT, mpcmp_tool_line *d_out, hipStream_t st) {
    if (nseg < 1 || 3 * nseg + 1 > TL_MAX_NODES || B < 1 || col_q < 0 || col_q + 7 > nx || col_v < 0 || col_v + 7 > nx || col_u < 0 || col_u + 7 > nu ||
        spec.n_sub < 1 || spec.n_sub > 64)
        return hipErrorInvalidValue;
    TlQRows qr;
    for (int j = 0; j < 7; j++) { qr.lb[j] = table.lbx[j]; qr.ub[j] = table.ubx[j]; }
    hipLaunchKernelGGL(k_tool_line, dim3((unsigned)((B + TL_NT - 1) / TL_NT)), dim3(TL_NT), 0, st, mdl, nseg, B, rows, qr, nx, nu, col_q, col_v, col_u,
                       d_q, d_R1, d_p1, d_Tin, spec, d_sx, d_su, d_sT, d_out);
    return hipGetLastError();
}

hipError_t tool_deviation_launch(const mpcmp_model *mdl, int nseg, int B, int nx, int col_q, const double *d_sx, const double *d_R1, const double *d_p1,
                                 int n_pts, double tol_lin, double tol_ang, mpcmp_tool_dev *d_out, hipStream_t st) {
    if (nseg < 1 || 3 * nseg + 1 > TL_MAX_NODES || B < 1 || col_q < 0 || col_q + 7 > nx || n_pts < 1 || n_pts > TD_MAX_PTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tool_deviation, dim3(B), dim3(TD_NT), 0, st, mdl, nseg, nx, col_q, d_sx, d_R1, d_p1, n_pts, tol_lin, tol_ang, d_out);
    return hipGetLastError();
}

}  // namespace mpcmp_tl
