/* mpcmp_limits.h — the between-node limit checker of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model, mpcmp_info,
 * mpcmp_bounds and mpcmp_clearance, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_LIMITS_H
#define MPCMP_LIMITS_H

/* ---- limits between the nodes: excess per group, the stretch that cures it, and the selection that reads it ----
 * The OCP enforces its bounds at the N collocation nodes; what a robot receives is the interpolant between them (mpcmp_sample_batch), and a cubic
 * through nodes that ride a bound leaves it in between.  Like the clearance checks this is a CHECKER of finished trajectories: no solve, warm start
 * or receding-horizon entry point reads any of it, a context that never calls these entry points behaves bit for bit as before, and mpcmp_create
 * allocates nothing for them.  Both arm layouts, every num_seg.
 * Per problem b the kernel takes the n_pts + 1 uniform normalised times ip / n_pts of mpcmp_sample_batch (the same Lagrange rule), 1 <= n_pts <=
 * 4096, and per (sample, arm) forms q, qd, qdd, the RNEA torque with that arm's model (the payload row of problem b, when payload rows are in force,
 * exactly as a solve reads it), the tool position and the world-aligned tool twist J(q) qd.  Samples are not stored.
 * Bounds in force: row b of mpcmp_set_bounds[_device] once rows are set, else the six tables of the configuration; in a two-arm context the row
 * applies to every arm.  Time windows, obstacles and multipliers are not read.
 * Groups and their channels.  For a value x with bounds [lb, ub] the excess is max(x - ub, lb - x): negative = inside by that much.
 *   MPCMP_LIM_Q         q[j]      against lbx[j], ubx[j]            channel 7 arm + j
 *   MPCMP_LIM_QD        qd[j]     against lbx[7 + j], ubx[7 + j]    channel 7 arm + j
 *   MPCMP_LIM_QDD       qdd[j]    against lbu[j], ubu[j]            channel 7 arm + j
 *   MPCMP_LIM_TAU       tau[j]    against lbg[j], ubg[j]            channel 7 arm + j
 *   MPCMP_LIM_HEIGHT    tool z (the eighth path row of mpcmp_eval_constraints_batch) against lbg[7], ubg[7]      channel arm
 *   MPCMP_LIM_TOOL_LIN  |linear part of J qd| - tool_lin_max                                                      channel arm
 *   MPCMP_LIM_TOOL_ANG  |angular part of J qd| - tool_ang_max                                                     channel arm
 * excess[g] is the maximum over samples, arms and channels; ties go to the lowest sample, then the lowest channel.  A group whose bounds are all
 * infinite (a tool maximum of +inf) reports excess -inf, t_at -1, channel -1.
 * stretch.  Collocation is in normalised time: stretching T by s divides every interpolated velocity and tool twist by s and every acceleration by
 * s^2.  Ratio of a velocity or acceleration value x: x / ub if x > 0, x / lb if x < 0, 0 if x == 0 or that bound is infinite, +inf if the bound on
 * x's side cannot be met by slowing down (ub <= 0 < x or lb >= 0 > x); of a tool speed: |v| / maximum, 0 for an infinite maximum (and for v == 0),
 * +inf for a maximum of 0 with v > 0.  With r_v, r_a, r_lin, r_ang the maxima over samples, arms and channels,
 *   stretch = max(1, r_v, sqrt(r_a), r_lin, r_ang);            tol is not read for it.
 * POSITIONS, TORQUES AND HEIGHT ARE NOT CURED BY A STRETCH (the torque has a gravity part that no slowing down removes; the path stays where it is).
 * For a move between states at rest, mpcmp_time_scale_batch to T * stretch makes QD, QDD, TOOL_LIN and TOOL_ANG hold.  With moving ends that call
 * replaces the end nodes by x0 / xf (see its own remark: a stretch is exact only between states at rest) and the statement is approximate.
 * A record does not depend on the launch, on the problem's position in the batch or on the batch around it (maxima by (value, key) compares, integer
 * sums and minima; no floating-point atomics).  LDS use does not grow with n_pts. */
#define MPCMP_LIM_GROUPS   7
#define MPCMP_LIM_Q        0
#define MPCMP_LIM_QD       1
#define MPCMP_LIM_QDD      2
#define MPCMP_LIM_TAU      3
#define MPCMP_LIM_HEIGHT   4
#define MPCMP_LIM_TOOL_LIN 5
#define MPCMP_LIM_TOOL_ANG 6
#define MPCMP_LIM_NAN      128   /* status bit: a non-finite sample value */
typedef struct { double tol[7]; double tool_lin_max, tool_ang_max; } mpcmp_limits_spec;   /* NULL spec: tol 0, both maxima +inf */
typedef struct {
    double excess[7];   /* per group, as above */
    double t_at[7];     /* physical time ip / n_pts * sol_T[b] of that sample */
    double stretch;     /* >= 1, above */
    double t_first;     /* time of the first sample at which some group's excess of that sample > its tol; -1 if none */
    int    channel[7];
    int    n_viol;      /* number of such samples */
    int    status;      /* bit g set iff excess[g] > tol[g]; MPCMP_LIM_NAN: a non-finite sample value (every excess NaN, the rest as for no bound) */
    int    pad;
} mpcmp_limits;         /* 168 bytes */
/* sol_x [B][N][14 narm], sol_u [B][N][7 narm], sol_T [B]; out [B].  Synchronous.  MPCMP_EINVAL, writing nothing: B < 1 or above max_batch, n_pts
 * outside [1, 4096], a required pointer NULL (spec may be NULL), more problems than bound rows or payload rows in force, a tol that is not finite, a
 * tool maximum that is NaN or negative. */
int mpcmp_limits_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T, int n_pts,
                       const mpcmp_limits_spec *spec, mpcmp_limits *out);
/* the arrays in DEVICE memory; spec stays a host pointer and is passed to the kernel by value.  Ordered on hip_stream, allocates nothing; checks the
 * scalars, the spec and the pointers against NULL, nothing the pointers point at */
int mpcmp_limits_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_pts,
                              const mpcmp_limits_spec *spec, mpcmp_limits *d_out, void *hip_stream);
/* ONE configuration on the host (no context, no GPU), with the arithmetic of the kernel: q, qd, qdd [7 narm] under the bounds `row` and `spec` (may
 * be NULL) -> excess [7], channel [7] (may be NULL) as above and ratios [4] (may be NULL) = the r_v, r_a, r_lin, r_ang terms of this configuration */
int mpcmp_limits_config(const mpcmp_model *models, int narm, const mpcmp_bounds *row, const mpcmp_limits_spec *spec, const double *q,
                        const double *qd, const double *qdd, double *excess, int *channel, double *ratios);
/* mpcmp_select_clear_batch with two changes: clr may be NULL (no clearance test), and a member is also inadmissible if lim != NULL and
 * (lim[i].status & (lim_mask | MPCMP_LIM_NAN)) != 0.  With lim == NULL and clr given it returns exactly what mpcmp_select_clear_batch returns; it
 * shares that call's scratch and its one-stream-at-a-time rule. */
int mpcmp_select_checked_batch(mpcmp_ctx *ctx, int B, const double *sol_T, const mpcmp_info *info, const mpcmp_clearance *clr,
                               const mpcmp_limits *lim, int lim_mask, const int *group, int n_groups, int *chosen);
int mpcmp_select_checked_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_T, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                      const mpcmp_limits *d_lim, int lim_mask, const int *d_group, int n_groups, int *d_chosen, void *hip_stream);

#endif  /* MPCMP_LIMITS_H */
