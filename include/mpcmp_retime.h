/* mpcmp_retime.h — retiming of finished plans, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model, mpcmp_bounds
 * and the group numbers of mpcmp_limits.h, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_RETIME_H
#define MPCMP_RETIME_H

/* ---- retiming: slow a finished plan only where it leaves its limits ----
 * The limit checker (mpcmp_limits.h) measures what a plan does between its nodes and offers one cure, `stretch`, a factor for the whole move.  This
 * is the finer cure: a time-optimal re-parameterisation of the plan ALONG ITS OWN PATH that holds the velocity, acceleration, torque and tool-speed
 * limits at every point of a grid and never runs faster than rate_max times the plan.  Like the limit checker it reads finished trajectories only:
 * no solve, warm start or receding-horizon entry point reads any of it, a context that never calls these entry points behaves bit for bit as
 * before, and mpcmp_create allocates nothing for them.  Both arm layouts, every num_seg.  THERE ARE NO JERK LIMITS: the rate is piecewise linear in
 * x below, so the acceleration of the retimed motion jumps at grid points.
 *
 * Path.  The project's three interpolants at the normalised s in [0, 1]: q(s), v(s), a(s) from the position, velocity and control nodes by the
 * Lagrange rule of mpcmp_sample_batch (what mpcmp_limits_batch evaluates too).
 * Rate.  The retimed plan runs the path with the rate lambda(s) > 0; x = lambda^2, and x == 1 is the plan as solved.  With w = dx/ds and T = sol_T[b]
 *   q_new   = q(s)
 *   qd_new  = lambda v(s)
 *   qdd_new = x a(s) + (w / 2T) v(s)
 *   tau_new = RNEA(q, qd_new, qdd_new) = c + x (RNEA(q, v, a) - c) + (w / 2T) (RNEA(q, 0, v) - c),   c = RNEA(q, 0, 0)
 *   tool twist = lambda J(q) v
 * With x == 1 / sigma^2 everywhere this is the stretch rule of the limit checker.
 * Grid.  s_k = k / n_grid, k = 0 .. n_grid, 1 <= n_grid <= 4096, Delta = 1 / n_grid.  x is piecewise linear: w_k is constant on [s_k, s_k+1] and
 * x_k+1 = x_k + Delta w_k.
 * Rows at grid point k, each A w + B x + C <= 0, per arm and joint j, with the bound tables of mpcmp_limits.h (row b of mpcmp_set_bounds once rows
 * are set, else the configuration's; in a two-arm context the row applies to every arm and the arms share x; the torque uses the payload row of
 * problem b when payload rows are in force):
 *   QDD upper   A =  v_j / 2T              B =  a_j                    C = -ubu[j]          QDD lower: -A, -B, C = lbu[j]
 *   TAU upper   A =  (RNEA(q,0,v) - c)_j / 2T    B = (RNEA(q,v,a) - c)_j     C = c_j - ubg[j]     TAU lower: -A, -B, C = lbg[j] - c_j
 * An infinite bound gives no row.  A coefficient with |A| <= 1e-12 (|B| + |C| + 1) is taken as 0 (at a state at rest v is exactly 0 and the RNEA
 * difference is rounding only).  A row with A == 0 bounds x alone: x <= -C / B for B > 0, x >= -C / B for B < 0, and with B == 0 it holds for every
 * x if C <= 0 and for none otherwise.
 * Caps (rows without w): x <= rate_max^2; per QD channel with v_j != 0, x <= (bound / v_j)^2 with the bound on v_j's side (ubx[7 + j] for v_j > 0,
 * lbx[7 + j] for v_j < 0), no cap for an infinite bound, cap 0 if that bound is <= 0 (>= 0 for the lower one); x <= (max / |J v|)^2 for the linear
 * and the angular part of the tool twist against tool_lin_max / tool_ang_max in the same way; and the rows whose A is 0.  cap_k is the least of them.
 * Q and HEIGHT are not read: no retiming cures them.  `groups` is a mask of the bits 1 << MPCMP_LIM_QD, QDD, TAU, TOOL_LIN, TOOL_ANG: the groups
 * that take part.
 * Ends.  An end of the plan (k = 0 or k = n_grid) at which some v_j != 0 in some arm keeps its speed: x is pinned to 1 there.  At k = n_grid only the
 * caps and the rows with A == 0 apply; the acceleration there is that of the interval before it.
 * Backward pass: controllable sets.  K_n = [lo_n, hi_n] from the caps and A == 0 rows of point n (lo_n = 0 without lower ones), or {1} if the end is
 * pinned.  For k < n, K_k = { x >= 0 : x <= cap_k, the A == 0 rows hold, and some w has rows_k(x, w) <= 0 and x + Delta w in K_k+1 } = [lo_k, hi_k].
 * It is computed exactly: the two next-state rows (A, B, C) = (Delta, 1, -hi_k+1) and (-Delta, -1, lo_k+1) join the rows of the point, and every
 * pair (row i with A_i > 0, row j with A_j < 0) leaves, w eliminated in product form,
 *   P x + Q <= 0,   P = A_i B_j - A_j B_i,   Q = A_i C_j - A_j C_i:    x <= -Q / P (P > 0),  x >= -Q / P (P < 0),  none feasible if P == 0 < Q.
 * The plan is INFEASIBLE if some K_k is empty, if hi_k == 0, or if a pinned end lies outside its set; k_fail is the point where the backward pass
 * met that (the highest such k; 0 for a pinned start outside K_0).
 * Forward pass.  x_0 = hi_0, or 1 if the start is pinned.  w_k = the least of -(B x_k + C) / A over the rows with A > 0, the next-state row
 * (hi_k+1 - x_k) / Delta included; x_k+1 = x_k + Delta w_k clipped into K_k+1.  What the profile stands for on interval k is w_k = (x_k+1 - x_k) n_grid.
 * Clock.  t_0 = 0, t_k+1 = t_k + 2 T Delta / (sqrt(x_k) + sqrt(x_k+1)) (exact: lambda is linear in time on an interval); T_new = t_n.  A clock that
 * is not finite (two neighbouring x of 0) reports the plan infeasible with k_fail = -1.
 * Retimed sample at the physical time t in [t_k, t_k+1]:  lambda = sqrt(x_k) + w_k (t - t_k) / 2T,  s = s_k + (t - t_k) (sqrt(x_k) + lambda) / 2T,
 * and the row is the formulas above at (s, lambda, w_k); the last sample is s = 1 with lambda = sqrt(x_n) and w_n-1.
 * A record and a profile do not depend on the launch, on the problem's position in the batch or on the batch around it: the two passes are
 * sequential, their minima and maxima are exact, and there are no atomics.  LDS use does not grow with n_grid. */
#define MPCMP_RT_INFEASIBLE 1     /* status bit: no rate within the limits (above) */
#define MPCMP_RT_NAN        128   /* status bit: a non-finite node value or a sol_T that is not finite and > 0 */
#define MPCMP_RT_ALL_GROUPS ((1 << MPCMP_LIM_QD) | (1 << MPCMP_LIM_QDD) | (1 << MPCMP_LIM_TAU) | (1 << MPCMP_LIM_TOOL_LIN) | (1 << MPCMP_LIM_TOOL_ANG))
typedef struct {
    double tool_lin_max, tool_ang_max;   /* >= 0, +inf: none */
    double rate_max;                     /* finite, > 0: lambda <= rate_max (1: never faster than the plan) */
    int    groups;                       /* mask, above */
    int    pad;
} mpcmp_retime_spec;                     /* 32 bytes.  NULL spec: +inf, +inf, 1, MPCMP_RT_ALL_GROUPS */
typedef struct {
    double T_new;       /* t_n */
    double rate_min;    /* min_k sqrt(x_k) */
    double s_slowest;   /* the s_k of that minimum; ties go to the lowest k */
    int    k_fail;      /* -1, or the grid point at which the backward pass failed */
    int    n_slowed;    /* number of grid points with x_k < rate_max^2 */
    int    status;      /* MPCMP_RT_INFEASIBLE, MPCMP_RT_NAN.  With either set: T_new +inf, rate_min 0, s_slowest -1, n_slowed 0, the profile NaN */
    int    pad;
} mpcmp_retime;         /* 40 bytes */
/* sol_x [B][N][14 narm], sol_u [B][N][7 narm], sol_T [B]; prof [B][n_grid + 1][2] = (t_k, x_k); out [B].  Synchronous.  MPCMP_EINVAL, writing
 * nothing: B < 1 or above max_batch, n_grid outside [1, 4096], a required pointer NULL (spec may be NULL), more problems than bound rows or payload
 * rows in force, a tool maximum that is NaN or negative, a rate_max that is not finite or <= 0, a groups bit outside MPCMP_RT_ALL_GROUPS. */
int mpcmp_retime_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid,
                       const mpcmp_retime_spec *spec, double *prof, mpcmp_retime *out);
/* the arrays in DEVICE memory; spec stays a host pointer and is passed to the kernel by value.  Ordered on hip_stream, allocates nothing; checks the
 * scalars, the spec and the pointers against NULL, nothing the pointers point at */
int mpcmp_retime_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_grid,
                              const mpcmp_retime_spec *spec, double *d_prof, mpcmp_retime *d_out, void *hip_stream);
/* ONE trajectory on the host (no context, no GPU), with the row, pair and clock arithmetic of the kernel: x [N][14 narm], u [N][7 narm] with
 * N = 3 num_seg + 1 (num_seg in 1 .. 8) under the bounds `row` and `spec` (may be NULL) -> prof [n_grid + 1][2], out [1] */
int mpcmp_retime_one(const mpcmp_model *models, int narm, int num_seg, const mpcmp_bounds *row, const mpcmp_retime_spec *spec, const double *x,
                     const double *u, double T, int n_grid, double *prof, mpcmp_retime *out);
/* The retimed plans at n_pts + 1 uniform PHYSICAL times: out [B][n_pts + 1][1 + 28 narm], a row = the time i T_new / n_pts, then per arm q, qd, qdd,
 * tau (7 each) by the retimed-sample rule above; prof and n_grid as a retime call left them.  A problem whose profile is NaN gets NaN rows.  THE
 * FIRST SAMPLER THAT ACCEPTS A TWO-ARM PLAN (mpcmp_sample_batch is for one arm).  The torque uses the payload rows in force.  MPCMP_EINVAL: B < 1 or
 * above max_batch, n_grid outside [1, 4096], n_pts < 1, a pointer NULL, more problems than payload rows. */
int mpcmp_sample_retimed_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid,
                               const double *prof, int n_pts, double *out);
int mpcmp_sample_retimed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_grid,
                                      const double *d_prof, int n_pts, double *d_out, void *hip_stream);

#endif  /* MPCMP_RETIME_H */
