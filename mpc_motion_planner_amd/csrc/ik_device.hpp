// ik_device.hpp — batched tool-pose targets (mpcmp_pose_targets_batch[_device], include/mpcmp.h): multi-start damped least-squares
// inverse kinematics of PandaWrapper::inverse_kinematic (robot_utils/pandaWrapper.cpp:14-60) for B problems x S starts, the choice of one
// start per problem under the joint bounds, and the joint velocity of PandaWrapper::inverse_velocities at that start.
//
// One lane per (problem, start).  A problem's starts sit in P adjacent lanes of one wave, P = S rounded up to a power of two (<= 64); the
// lanes beyond S take no part in the choice.  Every lane runs the host's DLS step (kinematics_host.hpp, one source for both) until its start
// converges or hits the cap; the wave runs as long as its slowest lane.  The choice is a butterfly of __shfl_xor over the P lanes on the key
// (class, value, start) — class 0: qualifying (value ||q - q_ref||^2, or 0 without q_ref), 1: not qualifying (value err), 2: padding lane —
// so every lane ends with the winner and no workspace or second kernel is needed.  The winning lane writes the target and the record.
// The model is read through wave-uniform addresses (scalar loads); the per-lane arrays of the step are indexed by unrolled constants only.
#pragma once
#include <hip/hip_runtime.h>
#include "kinematics_host.hpp"

namespace mpcmp {

struct IkBounds { double lq[7], uq[7], lv[7], uv[7]; };   // margin-applied position and velocity rows of lbx / ubx (one arm); `rows` of the kernel overrides them per problem

__global__ __launch_bounds__(256) void k_pose_targets(const mpcmp_model *__restrict__ model, IkBounds bd, const mpcmp_bounds *__restrict__ rows, int B, int S, int P, int nx, int col_q, int col_v,
                                                      const double *__restrict__ Rd, const double *__restrict__ pd, const double *__restrict__ twist,
                                                      const double *__restrict__ seeds, const double *__restrict__ q_ref, double *__restrict__ xf,
                                                      mpcmp_ik_info *__restrict__ info) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = (int)(t / P), s = (int)(t % P);
    if (b >= B) return;                          // whole groups only: P divides the wave, so no lane of a live group leaves here
    const mpcmp_model &M = *model;
    double R[9], p[3], q[7];
    for (int k = 0; k < 9; k++) R[k] = Rd[9 * (long)b + k];
    for (int k = 0; k < 3; k++) p[k] = pd[3 * (long)b + k];
    const bool live = s < S;
    for (int k = 0; k < 7; k++) q[k] = live ? seeds[(7 * ((long)b * S + s)) + k] : 0.0;
    double en = INFINITY;
    int it = 0;
    if (live)
        for (;; it++)
            if (mpcmp_host::ik_dls_step(M, R, p, q, it, &en) != mpcmp_host::IK_STEPPED) break;
    // wrap into the position rows; qualification and the key of the choice
    // (per-problem bounds, mpcmp_set_bounds: the problem's position and velocity rows instead of the configuration's, loaded where they are used:
    //  a per-lane copy of the four tables would live in 56 more registers through the whole iteration)
    bool inb = true;
    for (int j = 0; j < 7; j++) {
        const double lq = rows ? rows[b].lbx[j] : bd.lq[j], uq = rows ? rows[b].ubx[j] : bd.uq[j];
        q[j] = mpcmp_host::wrap_joint(q[j], lq, uq);
        inb = inb && q[j] >= lq && q[j] <= uq;
    }
    const bool conv = en < mpcmp_host::IK_EPS;
    int cls = !live ? 2 : (conv && inb ? 0 : 1);
    double val = 0.0;
    if (cls == 0 && q_ref) {
        for (int j = 0; j < 7; j++) { const double d = q[j] - q_ref[7 * (long)b + j]; val += d * d; }
    } else if (cls == 1) {
        val = en == en ? en : INFINITY;          // a NaN error ranks last
    }
    int idx = s;
    for (int off = 1; off < P; off <<= 1) {
        const int oc = __shfl_xor(cls, off);
        const double ov = __shfl_xor(val, off);
        const int oi = __shfl_xor(idx, off);
        if (oc < cls || (oc == cls && (ov < val || (ov == val && oi < idx)))) { cls = oc; val = ov; idx = oi; }
    }
    if (s != idx) return;
    int status = 0;
    if (cls != 0) status = (conv ? 0 : MPCMP_IK_NOT_CONVERGED) | (inb ? 0 : MPCMP_IK_Q_OUT_OF_BOUNDS);
    double qd[7] = {0, 0, 0, 0, 0, 0, 0};
    if (twist) {
        double v[6];
        for (int k = 0; k < 6; k++) v[k] = twist[6 * (long)b + k];
        if (!mpcmp_host::inverse_velocities(M, q, v, qd))
            for (int k = 0; k < 7; k++) qd[k] = NAN;
    }
    bool vin = true;
    for (int j = 0; j < 7; j++) vin = vin && qd[j] >= (rows ? rows[b].lbx[7 + j] : bd.lv[j]) && qd[j] <= (rows ? rows[b].ubx[7 + j] : bd.uv[j]);
    if (!vin) status |= MPCMP_IK_QD_OUT_OF_BOUNDS;
    double *row = xf + (long)b * nx;
    for (int j = 0; j < 7; j++) { row[col_q + j] = q[j]; row[col_v + j] = qd[j]; }
    if (info) {
        mpcmp_ik_info r;
        r.err = en; r.seed = idx; r.iters = it; r.status = status; r.pad = 0;
        info[b] = r;
    }
}

}  // namespace mpcmp
