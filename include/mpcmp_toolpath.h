/* mpcmp_toolpath.h — tool-line moves, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model and mpcmp_bounds, and
 * mpcmp.h includes it where they are known. */
#ifndef MPCMP_TOOLPATH_H
#define MPCMP_TOOLPATH_H

/* ---- tool-line moves: a straight Cartesian path written as a finished plan, and its checker ----
 * The generator writes the motion of one arm whose tool frame runs along a straight line (position) and a geodesic (orientation) into the arrays of
 * a finished plan, sol_x [B][N][14 narm], sol_u [B][N][7 narm], sol_T [B]: what mpcmp_limits_batch, mpcmp_clearance_batch, mpcmp_retime_batch,
 * mpcmp_sample_retimed_batch and (one arm) mpcmp_sample_batch read, and a legal start guess of mpcmp_solve_batch.  The checker says how far the
 * interpolant of the position nodes leaves that line between the nodes.  No solve, warm start or receding-horizon entry point reads any of it, a
 * context that never calls these entry points behaves bit for bit as before, and mpcmp_create allocates nothing for them.  Kinematic: payload rows
 * and time windows are not read.  Every num_seg, both arm layouts (one arm per call).
 *
 * Line.  (R0, p0) = the tool pose at q_start (the conventions of mpcmp_tool_jacobian), w = log(R0^T R1) (rotation vector),
 *   p(sigma) = p0 + sigma (p1 - p0),   R(sigma) = R0 exp(sigma [w]),   sigma in [0, 1];
 * the world twist per unit sigma is the constant V = [p1 - p0; R0 w].  The geodesic is ambiguous at a half turn: |w| > pi - 1e-3 is refused.
 * Progress.  sigma(s) = 10 s^3 - 15 s^4 + 6 s^5 on the plan's normalised time s: rest and zero acceleration at both ends, sigma' <= 15/8.
 * Duration.  T = T_in[b] where T_in is given and T_in[b] > 0; else T = max(15/8 |p1 - p0| / tool_lin_max, 15/8 |w| / tool_ang_max, T_min), so that
 * the nominal plan meets the two tool-speed maxima exactly at mid-move.  Joint limits are left to mpcmp_limits_batch and mpcmp_retime_batch.  The arms
 * of a two-arm plan share T, so there T_in is required (and a T_in[b] <= 0 still takes the rule, for this arm alone).
 * Velocity field.  g(q) = J^T (J J^T + damp I)^-1 V with the world-aligned J of mpcmp_tool_jacobian: the minimum-norm joint velocity per unit sigma.
 * Tracking.  q_0 = q_start.  Every interval between consecutive time nodes (mpcmp_time_nodes) is split into n_sub steps equal in sigma; a step is one
 * classical RK4 step of dq / dsigma = g(q) and then exactly two corrector steps q -= J^T (J J^T + damp I)^-1 e with e = [p - p(sigma);
 * log(R R(sigma)^T)] at the step's sigma.  The step count is fixed: no stop test decides it.
 * Stop rule.  At q_start and after every step: the pose error |e| and the manipulability m = sqrt(det(J J^T)).  Tracking stops if !(|e| <= eps), if
 * !(m >= manip_min) or if a normal matrix lost positive definiteness (each written so that a NaN stops).  k_fail is the node being approached (0 for
 * q_start); nodes k_fail .. N - 1 of q, v and u of this arm are NaN and MPCMP_TL_STOPPED is set.  The downstream checkers answer NaN nodes with their
 * own NaN bits.
 * Nodes.  With sd = sigma'(s_k) / T and sdd = sigma''(s_k) / T^2:  v_k = g(q_k) sd,  u_k = g(q_k) sdd + g'(q_k) sd^2, g' the derivative of g along
 * itself in closed form (A = J J^T + damp I, y = A^-1 V, J' = sum_i (dJ / dq_i) g_i:  g' = J'^T y - J^T A^-1 (J' J^T y + J J'^T y)).  v and u of the
 * first and the last node are exactly 0.  q, v, u are the nodes of the three interpolants of one smooth motion.
 * Position bounds.  The position rows of bound row b once mpcmp_set_bounds is in force, else the configuration's; q_excess is the largest of
 * lbx[j] - q_k[j], q_k[j] - ubx[j] over the nodes written (-inf if none or if every bound is infinite), and a positive one sets
 * MPCMP_TL_Q_OUT_OF_BOUNDS.  Nothing is wrapped: the path is continuous.
 * A plan and its record do not depend on the launch or on the problem's place in the batch: one lane per problem, no atomics. */
#define MPCMP_TL_STOPPED         1     /* status bit: tracking stopped at k_fail (above) */
#define MPCMP_TL_Q_OUT_OF_BOUNDS 2     /* status bit: q_excess > 0 */
#define MPCMP_TD_OVER            1     /* status bit of mpcmp_tool_dev: n_over > 0 */
#define MPCMP_TL_NAN             128   /* status bit of both records: a non-finite error, manipulability, duration or sample */
typedef struct {
    double tool_lin_max, tool_ang_max;   /* > 0, +inf: that term of the duration rule is 0 */
    double T_min;                        /* finite, > 0: the least duration the rule gives */
    double damp, manip_min, eps;         /* finite, > 0 */
    int    n_sub;                        /* 1 .. 64 */
    int    pad;
} mpcmp_tool_line_spec;                  /* 56 bytes.  NULL spec: 1.7, 2.5 (the tool maxima of mpcmp_traj_stats_batch), T_min 0.2, damp 1e-8,
                                          * manip_min 1e-3, eps 1e-9, n_sub 4.  T_min 0.2 s: the quintic's peak acceleration is 5.78 L / T^2, so a line
                                          * of a centimetre still starts with 1.5 m/s^2 instead of the 480 m/s^2 the tool-speed terms alone would give */
typedef struct {
    double err_max;      /* largest |e| met, the stopping one included */
    double manip_min;    /* least m met, the stopping one included */
    double s_manip;      /* where: s_k-1 + (j + 1) / n_sub (s_k - s_k-1) for step j of the interval before node k (0 for q_start); ties go to the first */
    double q_excess;     /* above */
    int    k_fail;       /* -1, or the node being approached when tracking stopped */
    int    status;       /* MPCMP_TL_STOPPED, MPCMP_TL_Q_OUT_OF_BOUNDS, MPCMP_TL_NAN */
} mpcmp_tool_line;       /* 40 bytes */
/* q_start [B][7], R1 [B][9] row-major, p1 [B][3], T_in [B] or NULL; sol_x [B][N][14 narm], sol_u [B][N][7 narm]: ONLY arm `arm`'s columns are written
 * (q at 7 arm, v at 7 narm + 7 arm of a state node, u at 7 arm of a control node), so a two-arm plan is two calls into one buffer, as for
 * mpcmp_pose_targets_batch; sol_T [B] is always written (T_in may be sol_T itself); out [B] may be NULL.  Synchronous.  MPCMP_EINVAL, writing nothing:
 * B < 1 or above max_batch, arm outside [0, narm), a required pointer NULL, a non-finite input value, an R1 that is not a rotation (the test of
 * mpcmp_pose_targets_batch), |w| > pi - 1e-3, n_sub outside [1, 64], a spec value that is not finite and > 0 (the tool maxima may be +inf), two arms
 * without T_in, more problems than bound rows in force. */
int mpcmp_tool_line_batch(mpcmp_ctx *ctx, int B, int arm, const double *q_start, const double *R1, const double *p1, const double *T_in,
                          const mpcmp_tool_line_spec *spec, double *sol_x, double *sol_u, double *sol_T, mpcmp_tool_line *out);
/* the arrays in DEVICE memory; spec stays a host pointer and is passed to the kernel by value.  Ordered on hip_stream, allocates nothing; checks the
 * scalars, the spec and the pointers against NULL, nothing the pointers point at (a half turn or a bad R1 there ends as a stopped or NaN plan) */
int mpcmp_tool_line_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_q_start, const double *d_R1, const double *d_p1, const double *d_T_in,
                                 const mpcmp_tool_line_spec *spec, double *d_sol_x, double *d_sol_u, double *d_sol_T, mpcmp_tool_line *d_out,
                                 void *hip_stream);
/* ONE line of one arm on the host (no context, no GPU), the same source as the kernel: x [N][14], u [N][7] with N = 3 num_seg + 1 (num_seg 1 .. 8),
 * *T, out [1] (may be NULL) under the position rows of `row`; T_in <= 0: the duration rule.  The value checks of mpcmp_tool_line_batch. */
int mpcmp_tool_line_one(const mpcmp_model *model, int num_seg, const mpcmp_bounds *row, const mpcmp_tool_line_spec *spec, const double *q_start,
                        const double *R1, const double *p1, double T_in, double *x, double *u, double *T, mpcmp_tool_line *out);

/* The checker: q of arm `arm` at the n_pts + 1 uniform s_i = i / n_pts by the Lagrange rule of mpcmp_sample_batch, its tool pose (R, p) by the forward
 * kinematics, against the nominal pose at sigma(s_i) of the line from (R0, p0) = the tool pose of node 0 to (R1, p1).  Per problem: the largest
 * distance |p - p(sigma(s_i))| and its s_i, the largest distance of p from the straight line through p0 and p1 (0 when |p1 - p0| <= 1e-9: such a line has no direction to working precision), the largest
 * rotation angle between R and R(sigma(s_i)) and its s_i (ties go to the lowest i), and the number of samples with a distance above tol_lin or an
 * angle above tol_ang.  THE DEVIATION IS A PROPERTY OF THE PATH, NOT OF THE CLOCK: a plan retimed by mpcmp_retime_batch runs through the same q(s), so
 * the record of the plan holds unchanged for the retimed plan (its samples lie at other s, between the ones checked here).
 * A non-finite sample: lin_max, perp_max, ang_max NaN, s_lin and s_ang -1, n_over 0, status MPCMP_TL_NAN.  A record does not depend on the launch
 * or on the problem's place in the batch: the maxima are exact and ordered by sample index, no atomics.  LDS use does not grow with n_pts. */
typedef struct {
    double lin_max, s_lin;     /* largest distance from the nominal position, and where */
    double perp_max;           /* largest distance from the straight line */
    double ang_max, s_ang;     /* largest angle from the nominal orientation, and where */
    int    n_over;             /* samples over tol_lin or tol_ang */
    int    status;             /* MPCMP_TD_OVER, MPCMP_TL_NAN */
} mpcmp_tool_dev;              /* 48 bytes */
/* sol_x [B][N][14 narm], R1 [B][9], p1 [B][3], out [B].  Synchronous.  MPCMP_EINVAL, writing nothing: B < 1 or above max_batch, arm outside
 * [0, narm), n_pts outside [1, 65536], a pointer NULL, a tolerance that is NaN or negative (+inf: never over). */
int mpcmp_tool_deviation_batch(mpcmp_ctx *ctx, int B, int arm, const double *sol_x, const double *R1, const double *p1, int n_pts, double tol_lin,
                               double tol_ang, mpcmp_tool_dev *out);
int mpcmp_tool_deviation_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_sol_x, const double *d_R1, const double *d_p1, int n_pts,
                                      double tol_lin, double tol_ang, mpcmp_tool_dev *d_out, void *hip_stream);
/* ONE plan of one arm on the host (no context, no GPU), the same source as the kernel: x [N][14] */
int mpcmp_tool_deviation_one(const mpcmp_model *model, int num_seg, const double *x, const double *R1, const double *p1, int n_pts, double tol_lin,
                             double tol_ang, mpcmp_tool_dev *out);

#endif  /* MPCMP_TOOLPATH_H */
