/*
 * mpcmp.h — C ABI of the MI355X-native batched minimum-time joint-space MPC solver.
 *
 * Drop-in boundary for the hot path of AlbericDeLajarte/mpc_motion_planner. The reference has no FFI
 * layer: its boundary is the C++ class `MotionPlanner` (mpc_solver/motionPlanner.hpp:16-176) whose
 * solve_trajectory() (mpc_solver/motionPlanner.cpp:177-208) calls polympc's mpc.solve() once per
 * (start,target) pair on one CPU thread (examples/benchmark.cpp:16 loops it 1000 times).  This ABI is what
 * a batched `MotionPlanner` binds instead; include/mpcmp_motion_planner.hpp is that binding.
 *
 * Conventions: every entry point returns 0 on success or a negative MPCMP_E* code and never throws; plain
 * pointers and sizes only; doubles everywhere (the reference is `double`, robot_ocp.hpp:38).  `*_device`
 * entry points take DEVICE pointers and a hipStream_t (as void*) and are asynchronous on that stream;
 * the others take HOST pointers and are synchronous.
 *
 * Layouts (node-major, ascending time — motionPlanner.cpp:158-174,202-203):
 *   x0, xf   [B][14]        = [q(7); qd(7)]            current_state / target_state (motionPlanner.hpp:40-41)
 *   sol_x    [B][N][14]     state at collocation node k  (mpc.solution_x(),  traj_state_t)
 *   sol_u    [B][N][7]      control (= qdd) at node k    (mpc.solution_u(),  traj_control_t)
 *   sol_T    [B]            final time                   (mpc.solution_p()[0])
 *   N = 3*num_seg + 1       (POLY_ORDER 3, robot_ocp.hpp:31-36)
 */
#ifndef MPCMP_H
#define MPCMP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MPCMP_NDOF 7
#define MPCMP_NX 14
#define MPCMP_NU 7
#define MPCMP_NG 8

#define MPCMP_OK 0
#define MPCMP_EINVAL (-1)      /* bad argument / unsupported configuration */
#define MPCMP_ENODEVICE (-2)   /* no HIP device, or the HIP runtime failed: the product has NO CPU fallback */
#define MPCMP_ERUNTIME (-3)    /* a HIP call failed; see mpcmp_last_error */
#define MPCMP_ETOOBIG (-4)     /* batch larger than the context's capacity */

typedef struct mpcmp_ctx mpcmp_ctx;

/* Serial chain of 7 revolute-z joints + tool frame; replaces pinocchio::Model built from the URDF
 * (robot_ocp.hpp:50-53, robot_utils/pandaWrapper.cpp:3-12). Same memory layout as the oracle's model. */
typedef struct {
    double R0[7][9];   /* fixed rotation of the joint placement (row-major), parent <- joint at q=0 */
    double p[7][3];    /* joint origin in the parent joint frame                                     */
    double mass[7];
    double com[7][3];  /* COM of the lumped body in its joint frame                                  */
    double I[7][9];    /* rotational inertia about the COM, in the joint frame, row-major.  All nine entries are read:
                        * I w is the row-major 3 x 3 product in every kernel (and in oracle/rbd.c).  A rigid body's tensor is
                        * symmetric; an asymmetric array is used as it stands, not symmetrised
                        * (tests/test_gpu_general_robot.py::test_inertia_is_read_row_by_row_vs_oracle)         */
    double tool[3];    /* frame "panda_tool" in the joint-7 frame (height constraint, robot_ocp.hpp:52,91) */
    double link8[3];   /* frame "panda_link8" in the joint-7 frame                                    */
    double gravity[3];
} mpcmp_model;

/* Solver settings + bounds; replaces mpc.settings()/qp_settings()/..._bounds() (motionPlanner.cpp:15-20,56-100).
 * mpcmp_create[_multi] and mpcmp_set_config reject with MPCMP_EINVAL: NaN or negative eps_abs, eps_rel, eps_target, hess_reg; rho_eq_scale <= 0;
 * ls_eta or ls_tau outside (0, 1); quirk_dtau_dT other than 0 / 1; in any bound pair NaN, lb > ub, lb = +inf or ub = -inf (infinite ends
 * otherwise switch a bound off); and for num_seg 1, 2, 4 a general row (lbg / ubg) narrower than 1e-4. */
typedef struct {
    int    num_seg;          /* NUM_SEG, robot_ocp.hpp:32 (4 -> 13 nodes, 6 -> 19 nodes as shipped, 8 -> 25)*/
    int    sqp_iters;        /* mpc.settings().max_iter,             motionPlanner.cpp:15 (2 as shipped)   */
    int    qp_iters;         /* mpc.qp_settings().max_iter,          motionPlanner.cpp:16 (700)            */
    int    ls_iters;         /* mpc.settings().line_search_max_iter, motionPlanner.cpp:17 (10)             */
    int    check_every;      /* ADMM termination-test interval (25)                                         */
    int    quirk_dtau_dT;    /* keep the non-physical d tau/dT column of robot_ocp.hpp:124,138 (1)          */
    double eps_abs, eps_rel; /* mpc.qp_settings().eps_*,             motionPlanner.cpp:19-20 (1e-3)        */
    double rho, sigma, alpha, rho_eq_scale;   /* box-ADMM parameters (0.02, 1e-6, 1.4, 1e3: fitted) */
    double ls_eta, ls_tau;   /* Armijo fraction and backtracking factor (0.25, 0.5)                         */
    double hess_reg;         /* Gershgorin shift, polympc_redef.hpp:68 (1e-3)                               */
    double eps_target;       /* terminal box half-width, motionPlanner.hpp:44 (1e-2)                        */
    double lbx[14], ubx[14]; /* mpc.state_bounds,       motionPlanner.cpp:66-70 */
    double lbu[7], ubu[7];   /* mpc.control_bounds,     motionPlanner.cpp:73    */
    double lbg[8], ubg[8];   /* mpc.constraints_bounds, motionPlanner.cpp:92-98 */
    double lbT, ubT;         /* mpc.parameters_bounds,  motionPlanner.cpp:76-79 */
    /* QP start of the SQP iterations after the first (the build's choice: polympc is absent).  0 (default) = every QP starts cold,
     * x = z = y = 0; 1 = warm duals: y_0 = the NLP multipliers lambda_k, x_0 = 0, z_0 = clip(0, l, u).  On the headline batch the warm start
     * nearly halves the ADMM iterations per trajectory with better feasibility; the stored reference solve is ONE SQP iteration
     * and cannot tell the two apart. */
    int    qp_warm_start;    /* also -1: off everywhere, including the receding-horizon driver (whose default is ON, see mpcmp_rh_run) */
    /* Multipliers at the start of a solve.  0 (default) = lambda_0 = 0 for every problem of every call (independent problems: the batch semantics).
     * 1 = the multipliers a problem slot was left with by the context's previous solve are the start of the next one (zero in a fresh context and
     * after mpcmp_reset_multipliers / mpcmp_rh_init): what a re-solve on ONE MotionPlanner object most plausibly does upstream (polympc keeps its
     * dual iterate until lam_guess is called: SURVEY.md 3.2, unverified) and what a receding-horizon loop wants.  Slot b of a call = problem b. */
    int    carry_multipliers; /* also -1: off everywhere, including the receding-horizon driver (whose default is ON, see mpcmp_rh_run) */
} mpcmp_config;

/* zero the carried multipliers of every problem slot (mpcmp_config.carry_multipliers) */
int mpcmp_reset_multipliers(mpcmp_ctx *ctx);

/* Per-problem result record; replaces mpc.info() (never read by the reference, motionPlanner.cpp:191). */
typedef struct {
    double T;             /* final time                                                   */
    double viol_l1;       /* l1 constraint violation of the returned iterate              */
    double defect_inf;    /* inf-norm of the collocation defects                          */
    double path_viol_inf; /* inf-norm violation of torque / height bounds at the nodes    */
    double term_err_inf;  /* || x_N - x_target ||_inf                                     */
    double last_alpha;    /* step length of the last SQP iteration                        */
    int    qp_iters_total;/* ADMM iterations executed over all SQP iterations             */
    int    sqp_iters;
    int    status;        /* 0 = converged QPs and an iterate inside every tolerance; else MPCMP_STATUS_* bits              */
    int    qp_capped;     /* number of SQP iterations whose QP ran out of qp_iters before its termination test was met    */
} mpcmp_info;
/* status bits.  The reference never reads mpc.info().status (motionPlanner.cpp:191); this record is the only failure channel a
 * batched caller has ("Failure detection"). */
#define MPCMP_STATUS_NAN          1   /* NaN / Inf in the returned iterate                                                   */
#define MPCMP_STATUS_NOT_PD       2   /* a KKT factorisation lost positive definiteness                                      */
#define MPCMP_STATUS_XCH_DEAD     4   /* multi-arm OCP: the partner workgroup never answered an exchange                     */
#define MPCMP_STATUS_QP_CAPPED    8   /* at least one QP stopped at qp_iters (qp_capped counts them): a truncated-ADMM step  */
#define MPCMP_STATUS_OUTSIDE_TOL 16   /* returned iterate outside tolerance: collocation defect or path violation > eps_abs,
                                         or terminal error > eps_target + eps_abs                                           */
#define MPCMP_STATUS_T_OUT_OF_BOX 32  /* final time outside [lbT, ubT]                                                       */
#define MPCMP_STATUS_ARRIVED      64  /* receding-horizon driver only: the instance has arrived and is no longer re-solved; the
                                         other bits and fields of the record are those of its last solve (mpcmp_rh_run)       */

/* ---- configuration helpers (host, no GPU needed) ---- */
int mpcmp_default_model(mpcmp_model *m);                                    /* Panda arm, panda_arm.urdf */
/* Payload: a rigid body attached to the flange, ADDED to whatever body 7 of a model already holds (the compiled-in Panda lumps its 1 kg tool
 * there).  mass >= 0; com and I (rotational inertia about the COM, row-major) in the joint-7 frame, the frame of mpcmp_model.tool and link8. */
typedef struct {
    double mass;
    double com[3];
    double I[9];
} mpcmp_payload;
/* body 7 of `m` with the payload lumped in (parallel-axis theorem, the arithmetic that lumps the Panda's fixed children); m == out is allowed.
 * A payload with mass 0 and I == 0 returns `m` unchanged, bit for bit.  Host and device (mpcmp_set_payloads*) results agree bit for bit.
 * MPCMP_EINVAL: mass < 0 or not finite, a non-finite com / I entry, I not symmetric, a negative diagonal entry of I. */
int mpcmp_model_add_payload(const mpcmp_model *m, const mpcmp_payload *p, mpcmp_model *out);
int mpcmp_model_from_urdf(const char *urdf_path, mpcmp_model *m);           /* MotionPlanner(std::string urdf_path), motionPlanner.cpp:3 */
/* General form (robot_utils/pandaWrapper.cpp:3-12 hands any URDF to Pinocchio): every serial chain of seven revolute joints that
 * hangs on the root link, in file order.  Fixed joints anywhere (rotated or not) are folded into the next joint placement and
 * their links lumped into the body of the joint frame they hang on; a chain's base placement is folded into its first joint;
 * rotated inertial frames and joint axes other than +z are handled.  *n_chains <= max_chains models are written; the result
 * feeds mpcmp_create_multi.  MPCMP_EINVAL (see mpcmp_last_error(NULL)): unsupported joint type, branching chain, != 7 joints. */
int mpcmp_models_from_urdf(const char *urdf_path, int max_chains, mpcmp_model *models, int *n_chains);
int mpcmp_default_limits(double *qmin, double *qmax, double *vmax, double *amax, double *jmax,
                         double *taumax);                                    /* pandaWrapper.hpp:29-34 */
int mpcmp_default_config(mpcmp_config *c, int num_seg, int sqp_iters);      /* motionPlanner.cpp:15-24 */
int mpcmp_set_margins(mpcmp_config *c, double margin_position, double margin_velocity,
                      double margin_acceleration, double margin_torque);    /* set_constraint_margins, motionPlanner.cpp:56-90 */
int mpcmp_set_min_height(mpcmp_config *c, double min_height);               /* set_min_height, motionPlanner.cpp:92-100 */
int mpcmp_num_nodes(int num_seg);
int mpcmp_time_nodes(int num_seg, double *tau);                             /* mpc.ocp().time_nodes, ascending */
const char *mpcmp_version(void);

/* ---- context ---- */
/* model == NULL -> compiled-in Panda. Allocates all device workspaces for up to max_batch problems;
 * no allocation happens in the solve calls. Fails with MPCMP_ENODEVICE when no GPU is present. */
int mpcmp_create(const mpcmp_config *cfg, const mpcmp_model *model, int device, int max_batch, mpcmp_ctx **out);
/* Multi-arm robot (BASELINE.json configs[3]: 14-DoF dual Panda): `models` points at narm (1 or 2) models — independent 7-joint
 * chains on one base; a chain's base placement is folded into its first joint placement (mpcmp_models_from_urdf).  The OCP is
 * the reference's (robot_ocp.hpp:31-213) with doubled sizes NX = 14 narm, NU = 7 narm, NG = 8 narm; the arms couple only
 * through the final time.  Layouts then are x0, xf [B][14 narm] = [q(7 narm); qd(7 narm)], sol_x [B][N][14 narm],
 * sol_u [B][N][7 narm]; the per-arm limit tables of mpcmp_config apply to every arm.  narm = 2 needs num_seg 6 or 8 and a warm
 * start (mpcmp_warm_start_jerk_batch[_device]); the leaf / resampling entry points are single-arm only. */
int mpcmp_create_multi(const mpcmp_config *cfg, const mpcmp_model *models, int narm, int device, int max_batch, mpcmp_ctx **out);
int mpcmp_destroy(mpcmp_ctx *ctx);
int mpcmp_set_config(mpcmp_ctx *ctx, const mpcmp_config *cfg);             /* num_seg must not change */
const char *mpcmp_last_error(const mpcmp_ctx *ctx);

/* ---- per-problem payloads ----
 * p [n][narm]: row i holds one payload per arm and applies to problem i (instance i of the receding-horizon driver, point i of the leaf calls)
 * of every later call that evaluates dynamics: mpcmp_solve_batch[_device], mpcmp_qp_batch, mpcmp_sample_batch[_device] (torque column),
 * mpcmp_mpc_point_batch, mpcmp_traj_stats_batch, mpcmp_rnea_batch, mpcmp_eval_constraints_batch and mpcmp_rh_init / mpcmp_rh_run.  Problem i is
 * solved with mpcmp_model_add_payload(model of the context, row i) for every arm.  Such a call with more problems than rows returns MPCMP_EINVAL
 * and writes nothing; so does mpcmp_rh_init with B > n.  The jerk-limited generators and mpcmp_pose_targets_* are kinematic and do not read the
 * rows.  n == 0 with p == NULL clears the rows (back to the context's model: outputs bit for bit those of a context that never set any).
 * mpcmp_set_payloads is synchronous and checks every row as mpcmp_model_add_payload does; it returns MPCMP_EINVAL, changing nothing, for n outside
 * [1, max_batch] (other than the clear), a bad row, or n below the B of a running receding-horizon loop.  Like mpcmp_set_config it drops a
 * captured receding-horizon graph (the next mpcmp_rh_run captures again); for the loop's instances see mpcmp_rh_update. */
int mpcmp_set_payloads(mpcmp_ctx *ctx, int n, const mpcmp_payload *p);
/* the same from DEVICE memory d_p [n][narm], ordered on hip_stream after the work already on it and before later work of the context; the values are
 * not read on the host and not checked (as mpcmp_rh_update_device) */
int mpcmp_set_payloads_device(mpcmp_ctx *ctx, int n, const mpcmp_payload *d_p, void *hip_stream);

/* ---- the hot path: B independent OCPs == B calls of MotionPlanner::solve_trajectory ---- */
/* warm_x/warm_u/warm_T: x_guess/u_guess/p_guess (motionPlanner.cpp:172-174); all NULL -> built-in
 * initialiser standing in for warm_start_RK (motionPlanner.cpp:146-175). info may be NULL. */
int mpcmp_solve_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf,
                      const double *warm_x, const double *warm_u, const double *warm_T,
                      double *sol_x, double *sol_u, double *sol_T, mpcmp_info *info);
int mpcmp_solve_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf,
                             const double *d_warm_x, const double *d_warm_u, const double *d_warm_T,
                             double *d_sol_x, double *d_sol_u, double *d_sol_T, mpcmp_info *d_info,
                             void *hip_stream);
/* built-in initialiser alone (what solve_batch uses when warm_* are NULL) */
int mpcmp_warm_start_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf,
                           double *warm_x, double *warm_u, double *warm_T);

/* ---- per-problem final-time windows ----
 * Row i = [lbT[i], ubT[i]] applies to problem i of every later mpcmp_solve_batch[_device], mpcmp_warm_start_batch, mpcmp_qp_batch and
 * mpcmp_solve_batch_synced[_device]: those calls read it wherever they read cfg.lbT / cfg.ubT (the box of T, the rho of the T row: a window narrower
 * than 1e-4 takes rho_eq, and MPCMP_STATUS_T_OUT_OF_BOX).  In a two-arm context the row applies to the problem; its arms share T.  Built-in
 * initialiser (warm_* NULL, and mpcmp_warm_start_batch): with rows set its geometric grid stops at the row's ubT instead of cfg.ubT, and a duration
 * below the row's lbT is raised to it (T = fmax(T, lbT) before the quintic's coefficients); without rows it is unchanged.  A caller's start guess is
 * never changed.  Such a call with more problems than rows returns MPCMP_EINVAL and writes nothing.  n == 0 with both pointers NULL clears the rows
 * (outputs bit for bit those of a context that never set any).  mpcmp_set_time_windows is synchronous; it returns MPCMP_EINVAL, changing nothing,
 * for n outside [1, max_batch] (other than the clear) and for a row that is not 0 <= lbT <= ubT, lbT < +inf, ubT > -inf (no NaN).  The receding-
 * horizon driver does not read the rows: with rows set mpcmp_rh_init returns MPCMP_EINVAL, and after mpcmp_rh_init both setters do. */
int mpcmp_set_time_windows(mpcmp_ctx *ctx, int n, const double *lbT, const double *ubT);
/* the same from DEVICE memory, ordered on hip_stream after the work already on it and before later work of the context; not checked */
int mpcmp_set_time_windows_device(mpcmp_ctx *ctx, int n, const double *d_lbT, const double *d_ubT, void *hip_stream);

/* ---- per-problem bounds ----
 * One row = the six bound tables of mpcmp_config, in the configuration's order (58 doubles, 464 bytes).  Row i applies to problem i of every later
 * mpcmp_solve_batch[_device], mpcmp_solve_batch_synced[_device] (both passes), mpcmp_qp_batch and mpcmp_warm_start_batch: those calls read the row
 * wherever they read the six tables of the configuration — the variable boxes, the path rows, the rho of a row or box (narrower than 1e-4 takes
 * rho_eq, so a locked joint, lbx[j] == ubx[j], changes the factor as well as the projection), viol_l1, path_viol_inf, MPCMP_STATUS_OUTSIDE_TOL and
 * the built-in initialiser's feasibility test (|qd| <= ubx[7 + j], |qdd| <= ubu[j]).  eps_target, the solver settings and [lbT, ubT] stay where
 * they are (configuration, final-time rows).  In a two-arm context a row applies to every arm of its problem, as the configuration's tables do.
 * mpcmp_pose_targets_batch[_device]: with rows set, rules 2, 3 and 5 (wrap, qualify, MPCMP_IK_QD_OUT_OF_BOUNDS) use problem i's position and velocity
 * rows, so that a target generated for a problem lies inside the box the problem is then solved in.
 * Not read by: the jerk-limited generators (the *_lim_* entry points take caller limits), the leaf calls, sampling, mpcmp_traj_stats_batch, the
 * clearance checks.  mpcmp_limits_batch[_device] (mpcmp_limits.h) checks problem i's interpolant under row i.
 * The receding-horizon driver does not read the rows either (its start guess comes from the generator with limits by value, and
 * a captured step holds kernel arguments): with rows set mpcmp_rh_init returns MPCMP_EINVAL, and after mpcmp_rh_init both setters do.
 * A call with more problems than rows returns MPCMP_EINVAL and writes nothing.  n == 0 with rows == NULL clears the rows: outputs then are bit for
 * bit those of a context that never set any.  The table (max_batch x 464 B) is allocated by the first setter call, never in a solve.
 * mpcmp_set_bounds is synchronous and applies to every row the rule the configuration's tables obey (mpcmp_create, mpcmp_set_config): in every pair
 * no NaN, lb <= ub, lb < +inf, ub > -inf; and for num_seg 1, 2, 4 a general row ubg - lbg >= 1e-4.  For a bad row, or n outside [1, max_batch]
 * (other than the clear), it returns MPCMP_EINVAL, names the row and field in mpcmp_last_error, and changes nothing.  mpcmp_set_config keeps working
 * with rows set: the rows win for the six tables. */
typedef struct { double lbx[14], ubx[14], lbu[7], ubu[7], lbg[8], ubg[8]; } mpcmp_bounds;
/* host helpers (no GPU needed): the configuration's six tables, bit for bit; and the tables of mpcmp_default_config + mpcmp_set_margins +
 * mpcmp_set_min_height(min_height), bit for bit */
int mpcmp_bounds_from_config(const mpcmp_config *c, mpcmp_bounds *out);
int mpcmp_bounds_from_margins(double margin_position, double margin_velocity, double margin_acceleration, double margin_torque,
                              double min_height, mpcmp_bounds *out);
int mpcmp_set_bounds(mpcmp_ctx *ctx, int n, const mpcmp_bounds *rows);
/* the same from DEVICE memory d_rows [n], ordered on hip_stream after the work already on it and before later work of the context; not checked */
int mpcmp_set_bounds_device(mpcmp_ctx *ctx, int n, const mpcmp_bounds *d_rows, void *hip_stream);

/* ---- time scaling of a trajectory ----
 * Collocation is in normalised time, so a solution stretched to T_new keeps its node positions.  Per problem b, exactly as the kernel computes it:
 *   s = sT[b] / T_new[b]                                   (one IEEE division)
 *   nodes 1 .. N-2:  ox[k][c] = sx[k][c]                   for c <  7 narm (joint positions)
 *                    ox[k][c] = sx[k][c] * s               for c >= 7 narm (joint velocities)
 *   node 0: ox[0] = x0[b];  node N-1: ox[N-1] = xf[b]     (the re-guess rule, motionPlanner.cpp:199-207: a stretch is exact only between states at rest)
 *                    (mpcmp_limits_batch's `stretch` is the factor of T that makes the kinematic limits hold between the nodes: exact under the same condition)
 *   every node:      ou[k][j] = su[k][j] * (s * s)
 *   oT[b] = T_new[b]
 * Layouts as mpcmp_solve_batch (x [B][N][14 narm], u [B][N][7 narm]); both arm layouts.  The outputs may be the inputs (ox == sx, ou == su,
 * oT == sT: every entry of a problem is formed from its inputs before oT is written). */
int mpcmp_time_scale_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *sx, const double *su, const double *sT,
                           const double *T_new, double *ox, double *ou, double *oT);
int mpcmp_time_scale_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_sx, const double *d_su,
                                  const double *d_sT, const double *d_T_new, double *d_ox, double *d_ou, double *d_oT, void *hip_stream);

/* ---- time-synchronised solve: independent problems of a group arrive together ----
 * 1. pass 1 = mpcmp_solve_batch[_device] with the same arguments and the rows in force.
 * 2. problem i is ELIGIBLE if 0 <= group[i] < n_groups and its pass-1 status has none of MPCMP_STATUS_NAN, _NOT_PD, _XCH_DEAD, _T_OUT_OF_BOX.
 *    group_T[g] = max of the pass-1 T over the group's eligible members (an order-independent atomic maximum: deterministic), NaN if it has none.
 *    group[i] == -1: not synchronised.  The host variant returns MPCMP_EINVAL for any other id outside [0, n_groups); the device variant treats
 *    such ids as -1.  n_groups in [0, max_batch].
 * 3. pass 2 re-solves every eligible member whose pass-1 T < group_T[g], from mpcmp_time_scale of its pass-1 solution to group_T[g], with the window
 *    [group_T[g], group_T[g]] (a context-internal row: the caller's rows do not change).  Multipliers follow carry_multipliers as in any solve.
 *    Every other problem keeps its pass-1 outputs bit for bit.
 * The device variant makes no host round trip: pass 2 is a launch over all B slots in which the problems not re-solved return at once (at N = 25 the
 * QP kernels still run for them, results discarded, and their status words are put back as pass 1 left them, so that the next solve of the context
 * (mpcmp_config.carry_multipliers, the re-guess rule) sees the state a plain solve leaves).  group_T [n_groups] or NULL; info may be NULL. */
int mpcmp_solve_batch_synced(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *warm_x, const double *warm_u,
                             const double *warm_T, const int *group, int n_groups,
                             double *sol_x, double *sol_u, double *sol_T, mpcmp_info *info, double *group_T);
int mpcmp_solve_batch_synced_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_warm_x, const double *d_warm_u,
                                    const double *d_warm_T, const int *d_group, int n_groups,
                                    double *d_sol_x, double *d_sol_u, double *d_sol_T, mpcmp_info *d_info, double *d_group_T, void *hip_stream);

/* ---- leaf kernels exposed for parity tests and for callers that only need the rigid-body layer ---- */
/* pinocchio::rnea (robot_ocp.hpp:91; motionPlanner.hpp:92,111,127,141): n x [q7],[qd7],[qdd7] -> n x [tau7] */
int mpcmp_rnea_batch(mpcmp_ctx *ctx, int n, const double *q, const double *qd, const double *qdd, double *tau);
/* minTime_ocp::evalConstraints AD overload (robot_ocp.hpp:98-163): n x [x14],[u7] -> g [n][8], G [n][8][22] */
int mpcmp_eval_constraints_batch(mpcmp_ctx *ctx, int n, const double *x, const double *u, double *g, double *G);
/* one QP of the SQP (linearise at (x,u,T,lam=0) + box-ADMM): p [B][21N+1] (layout xs|us|T), y [B][m+n],
 * iters [B]; m = 14(N-1) + 8N rows ordered [dynamics | path], then the n box rows. */
int mpcmp_qp_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *xs,
                   const double *us, const double *T, double *p, double *y, int *iters);

/* ---- resampling: MotionPlanner::get_MPC_trajectory<n_pts> (motionPlanner.hpp:99-116) ---- */
/* out [B][n_pts+1][29] = time, q(7), qd(7), qdd(7), tau(7) — the row format of analysis/optimal_solution.txt
 * (examples/offline_trajectory.cpp:88-105) */
int mpcmp_sample_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T,
                       int n_pts, double *out);
int mpcmp_sample_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_u,
                              const double *d_sol_T, int n_pts, double *d_out, void *hip_stream);

/* ---- jerk-limited, time-synchronised warm start (stands in for Ruckig, mpc_solver/motionPlanner.cpp:146-175) ----
 * Per joint: S-curve velocity transition, cruise, S-curve transition; minimum time of the slowest joint, every other joint
 * re-planned to exactly that duration.  Boundary accelerations: zero in the plain entry points (every example of the reference),
 * given in the *_acc_* ones (set_current_state / set_target_state forward them to Ruckig, motionPlanner.cpp:36-38,50-52).
 * Velocity / acceleration limits are the context's margin-applied bounds (mpcmp_set_margins), jmax[7] = margin_jerk *
 * max_jerk (motionPlanner.cpp:86-88).  Outputs in the layout mpcmp_solve_batch takes as warm start: warm_x [B][N][14],
 * warm_u [B][N][7], warm_T [B] (x_guess / u_guess / p_guess, motionPlanner.cpp:158-174). */
int mpcmp_warm_start_jerk_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax,
                                double *warm_x, double *warm_u, double *warm_T);
int mpcmp_warm_start_jerk_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *jmax,
                                       double *d_warm_x, double *d_warm_u, double *d_warm_T, void *hip_stream);
/* the same trajectory sampled uniformly, out [B][n_pts+1][22] = t, q(7), qd(7), qdd(7); T_out [B] (may be NULL):
 * MotionPlanner::get_ruckig_trajectory<n_pts> (motionPlanner.hpp:73-96) without the torque column block */
int mpcmp_jerk_trajectory_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, int n_pts,
                                double *out, double *T_out);

/* MotionPlanner::get_RK_point (motionPlanner.hpp:130-142): the same trajectory at ONE physical time per problem, clamped to
 * its duration, with the RNEA torque: out [B][28] = q(7), qd(7), qdd(7), tau(7); T_out [B] (may be NULL) = the durations. */
int mpcmp_jerk_point_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, const double *time,
                           double *out, double *T_out);
/* The three entry points above with boundary accelerations acc0 / accT [B][7] (either may be NULL = zero; with both NULL the result is
 * the plain entry point's bit for bit).  Single-arm contexts.  The acceleration limit yields to a given boundary acceleration above it.  A boundary
 * acceleration that drives a velocity from inside its limit to outside it however hard the jerk brakes (|v0| <= vmax < |v0 + a0 |a0| / 2J| at the start,
 * |vT| <= vmax < |vT - aT |aT| / 2J| at the target) is rejected with MPCMP_EINVAL by the host-pointer entry points, as Ruckig rejects such an input; the *_device variant does not read its inputs on the
 * host and does not check. */
int mpcmp_warm_start_jerk_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                    const double *jmax, double *warm_x, double *warm_u, double *warm_T);
int mpcmp_warm_start_jerk_acc_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_acc0, const double *d_accT,
                                           const double *jmax, double *d_warm_x, double *d_warm_u, double *d_warm_T, void *hip_stream);
int mpcmp_jerk_trajectory_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                    const double *jmax, int n_pts, double *out, double *T_out);
int mpcmp_jerk_point_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                               const double *jmax, const double *time, double *out, double *T_out);
/* The same three with the generator's velocity / acceleration limits given by the caller, vmax / amax [7] (either may be NULL = the context's
 * margin-applied bounds): what ruckig::InputParameter::max_velocity / max_acceleration are to otg.calculate (motionPlanner.cpp:149).  The
 * context's configuration is neither read for these limits nor changed. */
int mpcmp_warm_start_jerk_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                    const double *vmax, const double *amax, const double *jmax, double *warm_x, double *warm_u, double *warm_T);
int mpcmp_jerk_trajectory_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                    const double *vmax, const double *amax, const double *jmax, int n_pts, double *out, double *T_out);
int mpcmp_jerk_point_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                               const double *vmax, const double *amax, const double *jmax, const double *time, double *out, double *T_out);
/* MotionPlanner::get_MPC_point (motionPlanner.hpp:118-128): the solution at ONE physical time per problem, including the
 * reference's clamp (time >= T: the normalised time becomes T, not 1), with the RNEA torque: out [B][28] as above. */
int mpcmp_mpc_point_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T, const double *time,
                          double *out);

/* ---- scenario helpers of the robot wrapper (host side, as in the reference; never called by the batched solve) ---- */
/* World-aligned 6x7 Jacobian of the tool frame, rows [linear(3); angular(3)], row-major (J = blockdiag(R,R) * J_local,
 * robot_utils/pandaWrapper.cpp:70-75,97-101); optional tool position p[3] and rotation R[9] (row-major). */
int mpcmp_tool_jacobian(const mpcmp_model *model, const double *q, double *J, double *p, double *R);
/* PandaWrapper::forward_velocities (pandaWrapper.cpp:90-107): out[6] = J(q) qd = [linear; angular] task velocity. */
int mpcmp_forward_velocities(const mpcmp_model *model, const double *q, const double *qd, double *out);
/* PandaWrapper::inverse_velocities (pandaWrapper.cpp:62-88): qd = J^T (J J^T + 1e-5 I)^-1 [lin; ang]. */
int mpcmp_inverse_velocities(const mpcmp_model *model, const double *q, const double *lin, const double *ang, double *qd);
/* PandaWrapper::inverse_kinematic (pandaWrapper.cpp:14-60): damped least squares on the tool frame, error = log6 of the
 * pose error in the desired frame, step -J_local^T (J J^T + 1e-2 I)^-1 err * 0.1, stop at |err| < 1e-4 or 1000 iterations.
 * The reference starts from pinocchio::randomConfiguration; here the start q_init[7] is an argument (NULL = zeros).
 * R is row-major.  Returns MPCMP_OK when converged, 1 when the iteration cap was hit (q still holds the last iterate). */
int mpcmp_inverse_kinematics(const mpcmp_model *model, const double *R, const double *p, const double *q_init, double *q,
                             int *iters);

/* ---- batched tool-pose targets: multi-start inverse kinematics on the GPU ----
 * B problems, each a desired pose of the model's tool frame in the world frame (the frame of mpcmp_tool_jacobian): R [B][9] row-major,
 * p [B][3]; twist [B][6] the world-frame [linear; angular] tool velocity (NULL: qd = 0); q_seeds [B][S][7] the starts, 1 <= S <= 64;
 * q_ref [B][7] optional.  xf [B][14 narm] in the layout mpcmp_solve_batch and mpcmp_rh_update take; only arm `arm`'s 14 columns are
 * written: q at [7 arm, 7 arm + 7) and qd at [7 narm + 7 arm, 7 narm + 7 arm + 7) (a two-arm target is two calls into one buffer).
 * arm selects the context's model; info [B] may be NULL.  Rules:
 *   1. per start: the DLS loop of mpcmp_inverse_kinematics unchanged (eps 1e-4, IT_MAX 1000, DT 0.1, damp 1e-2, local-frame Jacobian);
 *   2. wrap: each joint j is shifted to q_j + 2 pi k with the integer k of smallest |k| that puts it into [lbx_j, ubx_j], k = 0 when none
 *      does; the bounds are the context configuration's margin-applied position rows (for two arms the per-arm rows apply to every arm), or
 *      problem i's row once mpcmp_set_bounds[_device] has set rows (B above their number: MPCMP_EINVAL);
 *   3. a start qualifies if it converged (err < 1e-4) and all 7 of its wrapped joints lie within the bounds;
 *   4. choice: if some start qualifies and q_ref is given, the qualifying start that minimises ||q - q_ref||_2 (wrapped q; ties to the
 *      lowest index); if some start qualifies and q_ref is NULL, the lowest qualifying index; if none qualifies, the smallest err (ties
 *      to the lowest index), with MPCMP_IK_NOT_CONVERGED and / or MPCMP_IK_Q_OUT_OF_BOUNDS set for that start;
 *   5. velocity: qd = J^T (J J^T + 1e-5 I)^-1 twist at the chosen, wrapped q with the world-aligned J (mpcmp_inverse_velocities);
 *      MPCMP_IK_QD_OUT_OF_BOUNDS if qd leaves the velocity rows of lbx / ubx.
 * The host-pointer variant is synchronous and returns MPCMP_EINVAL, writing nothing, for B < 1, S outside [1, 64], arm outside [0, narm),
 * a required pointer NULL, a value that is not finite, or an R that is not a rotation (max |(R^T R - I)_ij| > 1e-6 or det R <= 0).
 * The device variant checks only the scalars and NULL pointers and is ordered on hip_stream. */
typedef struct {
    double err;    /* ||log6(oMdes^-1 oMf)|| of the chosen start's last iterate */
    int    seed;   /* index of the chosen start */
    int    iters;  /* DLS iterations of the chosen start */
    int    status; /* 0 or MPCMP_IK_* bits */
    int    pad;
} mpcmp_ik_info;
#define MPCMP_IK_NOT_CONVERGED     1
#define MPCMP_IK_Q_OUT_OF_BOUNDS   2
#define MPCMP_IK_QD_OUT_OF_BOUNDS  4
int mpcmp_pose_targets_batch(mpcmp_ctx *ctx, int B, int arm, const double *R, const double *p, const double *twist,
                             int S, const double *q_seeds, const double *q_ref, double *xf, mpcmp_ik_info *info);
int mpcmp_pose_targets_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_R, const double *d_p, const double *d_twist,
                                    int S, const double *d_q_seeds, const double *d_q_ref, double *d_xf, mpcmp_ik_info *d_info,
                                    void *hip_stream);

/* ---- trajectory checks of the reference benchmark (examples/benchmark.cpp:58-160) ---- */
/* out [B][74] = min(28) | max(28) of q,qd,qdd,tau over n_pts+1 uniform samples | x(T) - target (14) |
 * flags (4; 1 = pass): jerk (|d qdd/dt| <= 10 max_jerk), linear task velocity <= 1.7, angular <= 2.5, tool z >= 0.
 * One 162-number row of analysis/benchmark_data.txt = [guess min, guess max, mpc min, mpc max, guess err, mpc err,
 * guess flags, mpc flags, target] (benchmark.cpp:164-194). */
int mpcmp_traj_stats_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T,
                           const double *xf, int n_pts, double *out);

/* ---- clearance: robot spheres against obstacles and against the other arm ----
 * A CHECKER of finished trajectories, not a constraint of the OCP: no solve, warm start or receding-horizon entry point reads any of this, and a
 * context that never calls the setters behaves bit for bit as one built without them.  mpcmp_create[_multi] adds one fixed-size table (128 sphere
 * records, 5 KB); obstacles are allocated by mpcmp_set_obstacles[_device] when they grow; mpcmp_clearance_batch_device allocates nothing;
 * mpcmp_select_clear_batch[_device] allocates its scratch (five arrays of max_batch entries) in its first call and nothing afterwards.
 * Streams.  The tables and the selection's scratch belong to the context, the *_device calls run on the caller's stream.  The synchronous setters
 * (mpcmp_set_robot_spheres, mpcmp_set_obstacles) wait for all work of the device before they write, so they may be called at any time.
 * mpcmp_set_obstacles_device is ordered against the context's own stream and hip_stream only: a check in flight on ANOTHER stream must be ordered
 * against it by the caller.  mpcmp_select_clear_batch_device uses one scratch per context: enqueue selections of one context on one stream at a
 * time (or order them with events); a context per stream has no such limit.
 * The robot is a set of spheres fixed to joint frames, the world a set of primitives.  Signed distance sd(x, obstacle) of a world point x:
 *   sphere      |x - a| - r
 *   capsule     t = clamp((x - a).(b - a) / |b - a|^2, 0, 1)  (t = 0 when a == b),  |x - a - t (b - a)| - r
 *   box         d = |x - a| - b componentwise,  |max(d, 0)| + min(max(d.x, d.y, d.z), 0) - r
 *   half-space  a.x - b[0]
 * Clearance of robot sphere s at world centre c_s: sd(c_s, obstacle) - r_s; of a robot pair: |c_s - c_t| - r_s - r_t.  World centres follow the chain
 * of the whole library: p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i), c_s = p_w[joint] + R_w[joint] c.
 * Pairs: every robot sphere x every obstacle; with two arms every sphere of arm 0 x every sphere of arm 1; and, if self_gap > 0, the spheres of one
 * arm whose joint indices differ by at least self_gap.  Spheres are numbered arm-major in table order; a robot pair is named (s, t) with s < t. */
typedef struct { int joint; int pad; double c[3]; double r; } mpcmp_sphere;
/* joint 0..6: centre c in the frame of that joint (the frame mpcmp_model.com[joint] is given in); r > 0 */
#define MPCMP_OBS_SPHERE    0   /* a = centre, r = radius                                                    */
#define MPCMP_OBS_CAPSULE   1   /* segment a..b, r = radius                                                  */
#define MPCMP_OBS_BOX       2   /* axis-aligned: a = centre, b = half extents (> 0), r >= 0 rounds the edges */
#define MPCMP_OBS_HALFSPACE 3   /* solid { x : a.x <= b[0] }, a = unit normal pointing into free space       */
typedef struct { int type; int pad; double a[3], b[3]; double r; } mpcmp_obstacle;   /* world frame */

/* host helpers (no GPU needed) */
/* A SKELETON sphere model from the model alone (not a fitted hull: it follows the lines between the joint origins and knows nothing of the link
 * shapes): for joint i = 0..5 spheres of radius `radius` on the segment from the origin of joint i to p[i+1], for joint 6 from its origin to `tool`
 * (all in joint i's frame); on a segment of length L, ceil(L / spacing) + 1 centres equally spaced including both ends (one when L == 0).
 * MPCMP_EINVAL, writing nothing: radius <= 0, spacing <= 0, more than `max` spheres. */
int mpcmp_link_spheres(const mpcmp_model *model, double radius, double spacing, int max, mpcmp_sphere *out, int *n);
/* minimum clearance of ONE configuration q [7 narm] on the host: the pair set, formulas and tie order of mpcmp_clearance_batch for one sample.
 * spheres [n_spheres[0] + .. ] arm-major; *sphere / *other (may be NULL) as in mpcmp_clearance; d_min = +inf, sphere = -1 when there is no pair. */
int mpcmp_clearance_config(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                           const mpcmp_obstacle *obs, int self_gap, const double *q, double *d_min, int *sphere, int *other);

/* sphere table of one arm: 0 <= n <= 64; n == 0 clears.  Synchronous.  MPCMP_EINVAL, changing nothing: arm outside [0, narm), n out of range, a joint
 * outside 0..6, a value that is not finite, r <= 0. */
int mpcmp_set_robot_spheres(mpcmp_ctx *ctx, int arm, int n, const mpcmp_sphere *spheres);
/* obs [n_sets][n_obs], n_obs <= 256.  n_sets == 1: one world for every problem.  n_sets > 1 (<= max_batch): set i applies to problem i, and a
 * clearance call with B > n_sets returns MPCMP_EINVAL and writes nothing.  n_sets == 0 (or n_obs == 0) clears.  The host variant is synchronous and
 * rejects, changing nothing: unknown types, values that are not finite, r < 0, box half extents <= 0, a half-space normal with | |a| - 1 | > 1e-9.
 * The device variant is ordered on hip_stream after the work already on it and before later work of the context; its values are not checked. */
int mpcmp_set_obstacles(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *obs);
int mpcmp_set_obstacles_device(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *d_obs, void *hip_stream);

typedef struct {
    double d_min;    /* smallest clearance over all samples and pairs (+inf when there is no pair)                          */
    double t_min;    /* physical time of that sample, ip / n_pts * sol_T[b] (-1 when there is no pair)                       */
    double t_first;  /* physical time of the first sample with a clearance < margin; -1 if none                             */
    int    sphere;   /* at d_min: robot sphere, numbered arm-major over the context's sphere tables (-1 when there is no pair) */
    int    other;    /* at d_min: obstacle index >= 0, or -1 - (index of the second robot sphere)                            */
    int    n_hit;    /* number of samples with some clearance < margin                                                       */
    int    status;   /* 0, MPCMP_CLR_HIT (n_hit > 0), MPCMP_CLR_NAN (a non-finite sample: d_min = NaN, the rest as for no pair) */
} mpcmp_clearance;
#define MPCMP_CLR_HIT 1
#define MPCMP_CLR_NAN 2
/* B trajectories sol_x [B][N][14 narm] (positions of arm a in columns [7a, 7a + 7)), sol_T [B], checked at the n_pts + 1 uniform normalised times of
 * mpcmp_sample_batch (the same Lagrange interpolation on the segment), 1 <= n_pts <= 4096; out [B].  Both arm layouts, every num_seg.  Ties of d_min:
 * lowest sample, then lowest sphere, then obstacles before robot pairs, then lowest index; a problem's record does not depend on the batch around
 * it.  Kinematic: payload rows and time windows are not read.  MPCMP_EINVAL, writing nothing: B < 1, n_pts out of range, a NULL pointer, margin not
 * finite, self_gap < 0, more problems than obstacle sets.  The forward kinematics run once per (problem, sample); the tables live in LDS, whose use
 * does not grow with n_pts. */
int mpcmp_clearance_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, int n_pts, double margin, int self_gap,
                          mpcmp_clearance *out);
int mpcmp_clearance_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, int n_pts, double margin, int self_gap,
                                 mpcmp_clearance *d_out, void *hip_stream);
/* "plan K candidates, keep the fastest one that hits nothing": group [B], n_groups in [0, max_batch] with the id rules of mpcmp_solve_batch_synced
 * (-1: in no group; the host variant returns MPCMP_EINVAL for other ids outside [0, n_groups), the device variant treats them as -1).  A member is
 * admissible if info[i].status has none of MPCMP_STATUS_NAN, _NOT_PD, _XCH_DEAD, _OUTSIDE_TOL, _T_OUT_OF_BOX and clr[i].status == 0.
 * chosen [n_groups] = the admissible member with the smallest sol_T, ties to the lowest problem index, -1 if the group has none.  Deterministic
 * (integer minima); the device variant makes no host round trip. */
int mpcmp_select_clear_batch(mpcmp_ctx *ctx, int B, const double *sol_T, const mpcmp_info *info, const mpcmp_clearance *clr, const int *group,
                             int n_groups, int *chosen);
int mpcmp_select_clear_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_T, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                    const int *d_group, int n_groups, int *d_chosen, void *hip_stream);

/* ---- limits between the nodes: excess per group, the stretch that cures it, and the selection that reads it ----
 * The checker of the limits themselves, beside the clearance checker: records, constants and entry points are declared in mpcmp_limits.h, which
 * needs the types above and is part of this interface. */
#include "mpcmp_limits.h"
#include "mpcmp_retime.h"
#include "mpcmp_toolpath.h"
#include "mpcmp_clearance_cert.h"
#include "mpcmp_moving.h"
#include "mpcmp_moving_cert.h"
#include "mpcmp_field.h"
#include "mpcmp_field_cert.h"
#include "mpcmp_frame.h"

/* ---- via-point routes: plan, join, sample and check multi-leg moves ----
 * A route is x0 -> via_0 -> .. -> via_{M-1} -> xf, passed without stopping.  With the joint state (q, qd) fixed at a via, the legs on either side are
 * independent minimum-time OCPs: a batch of B routes with M >= 0 vias is a batch of L = B (M + 1) ordinary problems, and LEG SLOT l = b (M + 1) + m
 * is leg m of route b.  The row tables (payloads, final-time windows, bounds) and the per-problem obstacle sets keep their one rule, row l applies to
 * batch slot l: for routes the batch slot is the leg slot, so a route under its own limits sets its row M + 1 times.  No solve kernel changes.
 * L > max_batch: MPCMP_EINVAL, nothing written.  All arithmetic is FP64 and every sum runs sequentially in leg order: a route's records do not depend
 * on the batch around it and are bitwise reproducible.  A context that never calls one of these entry points behaves bit for bit as before.
 * Points and velocities (nq = 7 narm): P_0 = q(x0[b]), P_i = via[b][i-1], P_{M+1} = q(xf[b]); V_0 = qd(x0[b]), V_{M+1} = qd(xf[b]); leg m runs from
 * (P_m, V_m) to (P_{m+1}, V_{m+1}).  V_1 .. V_M are via_qd when it is given (copied bit for bit), otherwise the CHORD RULE: with a = P_i - P_{i-1},
 * b = P_{i+1} - P_i, per column j
 *   vlim_j = min(ubx[7 + j], -lbx[7 + j]),  alim_j = min(ubu[j], -lbu[j])     of the bound row of the leg slot that STARTS at the via, or of the
 *                                                                              configuration without rows (per-arm tables: every arm's 7 columns)
 *   d_j = 0.5 (a_j + b_j)  if a_j b_j > 0 and vlim_j > 0 and alim_j > 0,  else 0   (a joint that reverses or rests at the via; a locked joint)
 *   s   = min over the j with d_j != 0 of  min(vlim_j, sqrt(2 alim_j min(|a_j|, |b_j|))) / |d_j|
 *   V_i = speed_b s d,  each entry then held to |V_j| <= vlim_j (against the rounding of the product);  V_i = 0 if every d_j is 0, or if s is
 *         infinite (every moving joint without limits: nothing to scale to)
 * The rule keeps the direction of the tangent; no joint passes faster than its limit, or faster than the speed it could reach over the shorter
 * neighbouring chord at its acceleration limit.  With M == 0 the one leg is (x0, xf) unchanged. */
/* the chord rule on the host (no GPU needed; the function the kernel runs): p_prev, p_via, p_next, v [7 narm]; speed in [0, 1] */
int mpcmp_route_via_velocity(const double *p_prev, const double *p_via, const double *p_next, const mpcmp_bounds *row, int narm, double speed,
                             double *v);
/* x0, xf [B][14 narm]; via [B][M][7 narm] (NULL with M == 0); via_qd [B][M][7 narm] or NULL; speed [B] or NULL (= 1).  leg_x0, leg_xf [L][14 narm];
 * via_qd_out [B][M][7 narm] may be NULL.  The host-pointer variant returns MPCMP_EINVAL, writing nothing, for B < 1, M < 0, L > max_batch, a required
 * pointer NULL, a value that is not finite, a speed outside [0, 1], fewer bound rows than leg slots; the device variant does not read its inputs on
 * the host.  Both return MPCMP_EINVAL after mpcmp_rh_init. */
int mpcmp_route_legs(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed, const double *xf,
                     double *leg_x0, double *leg_xf, double *via_qd_out);
int mpcmp_route_legs_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_via_qd, const double *d_speed,
                            const double *d_xf, double *d_leg_x0, double *d_leg_xf, double *d_via_qd_out, void *hip_stream);
/* Join: the legs' outputs sol_x [B][M+1][N][14 narm], sol_u [B][M+1][N][7 narm], sol_T [L], info [L] and optionally clr [L] (with route_clr [B];
 * both NULL otherwise) as one record per route, in the types mpcmp_select_clear_batch[_device] takes.
 *   route_T [B], route_info [B]: T = the sum of the legs' sol_T, m = 0 .. M; viol_l1, defect_inf, path_viol_inf, term_err_inf and sqp_iters maxima
 *     over the legs, last_alpha the minimum (a NaN stays); qp_iters_total and qp_capped sums; status the OR of the legs' bits.
 *   seam [B]: state_jump_inf = the largest |last node of leg m - node 0 of leg m + 1| over the vias and the columns of sol_x, acc_jump_inf the same
 *     over sol_u (both 0 with M == 0); leg_longest = the leg with the largest T, ties to the lowest; leg_first_bad = the lowest leg whose status has a
 *     bit of mpcmp_select_clear_batch's inadmissible set, -1 if none.  ACCELERATIONS ARE NOT CONTINUOUS AT A VIA: position and velocity are fixed
 *     there, the acceleration is each leg's own, and acc_jump_inf says by how much they differ (a tracking controller sees a torque step there).
 *   route_clr [B]: d_min = the minimum over the legs that have a pair, ties to the lowest leg, sphere and other from that leg, t_min = that leg's
 *     t_min + the sum of the earlier legs' T; t_first from the lowest leg that has one, shifted the same way; n_hit the sum (a junction sample belongs
 *     to both legs and is counted in both); status the OR.  If any leg has MPCMP_CLR_NAN: d_min = NaN, t_min = t_first = -1, sphere = -1, other = 0,
 *     n_hit = 0, status still the OR.  If no leg has a pair, the "no pair" record of mpcmp_clearance.
 * One thread per route.  MPCMP_EINVAL, writing nothing: B < 1, M < 0, L > max_batch, a required pointer NULL, exactly one of clr / route_clr given. */
typedef struct {
    double state_jump_inf;
    double acc_jump_inf;
    int    leg_longest;
    int    leg_first_bad;
} mpcmp_route_seam;
int mpcmp_route_join(mpcmp_ctx *ctx, int B, int M, const double *sol_x, const double *sol_u, const double *sol_T, const mpcmp_info *info,
                     const mpcmp_clearance *clr, double *route_T, mpcmp_info *route_info, mpcmp_route_seam *seam, mpcmp_clearance *route_clr);
int mpcmp_route_join_device(mpcmp_ctx *ctx, int B, int M, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, const mpcmp_info *d_info,
                            const mpcmp_clearance *d_clr, double *d_route_T, mpcmp_info *d_route_info, mpcmp_route_seam *d_seam,
                            mpcmp_clearance *d_route_clr, void *hip_stream);
/* Solve, in this order: 1. the leg builder into context scratch (allocated by the first call, never afterwards); 2. the start guess of the legs:
 * mpcmp_warm_start_jerk_batch_device on the leg states when jmax [7] (a HOST pointer in both variants) is given, the built-in initialiser when it is
 * NULL (two-arm contexts need jmax); 3. ONE ordinary solve of the L legs with the rows in force: the leg outputs are bit for bit those of
 * mpcmp_solve_batch[_device] on (leg_x0, leg_xf) with that start guess; 4. the join.  Outputs: the legs' sol_x, sol_u, sol_T [L] and info [L] (may be
 * NULL), route_T, route_info, seam [B], via_qd_out (may be NULL).  Both arm layouts, every num_seg of the context.  The device variant makes no host
 * round trip and is ordered on hip_stream; the scratch belongs to the context: enqueue route solves of one context on one stream at a time.
 * MPCMP_EINVAL, writing nothing: as mpcmp_route_legs, fewer rows of any table than leg slots, and after mpcmp_rh_init (as the row setters). */
int mpcmp_solve_route_batch(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                            const double *xf, const double *jmax, double *sol_x, double *sol_u, double *sol_T, mpcmp_info *info,
                            double *route_T, mpcmp_info *route_info, mpcmp_route_seam *seam, double *via_qd_out);
int mpcmp_solve_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_via_qd, const double *d_speed,
                                   const double *d_xf, const double *jmax, double *d_sol_x, double *d_sol_u, double *d_sol_T, mpcmp_info *d_info,
                                   double *d_route_T, mpcmp_info *d_route_info, mpcmp_route_seam *d_seam, double *d_via_qd_out, void *hip_stream);
/* Sampling on a uniform clock across the junctions (single-arm contexts, as mpcmp_sample_batch): out [B][n_pts+1][29] = route time, q, qd, qdd, tau.
 * R = the sequential sum of the legs' T, E_m its prefix sum after leg m (E_-1 = 0).  Sample i has t = (double)i / n_pts * R; its leg is the smallest m
 * with t < E_m, M if there is none; its normalised time is clamp((t - E_{m-1}) / T_m, 0, 1) (0 where the quotient is no number); sample n_pts is leg
 * M at exactly 1.  A junction sample belongs to the LATER leg at normalised time 0.  The row is the one mpcmp_sample_batch gives for that leg there
 * (one device function: the same Lagrange interpolation, RNEA with the payload row of the leg slot).  A route with a leg T that is not finite gets
 * NaN rows.  mpcmp_route_locate is the leg / normalised-time rule on the host (no GPU needed; the function the kernel runs). */
int mpcmp_route_locate(int n_legs, const double *leg_T, double t, int *leg, double *tau);
int mpcmp_sample_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sol_x, const double *sol_u, const double *sol_T, int n_pts, double *out);
int mpcmp_sample_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_pts,
                                    double *d_out, void *hip_stream);
#include "mpcmp_route_retime.h"
#include "mpcmp_retimed_check.h"

/* ---- receding-horizon driver (BASELINE.json config #5) ---- */
/* B instances; every step = re-solve warm-started from the previous solution with the reference's re-guess rule
 * (head := current state, tail := target; motionPlanner.cpp:199-207), then the current state advances along the
 * new solution by dt (MotionPlanner::get_MPC_point, motionPlanner.hpp:118-128).  The first step starts from the
 * jerk-limited trajectory (below).  use_graph != 0 replays one hipGraph-captured step (fixed iteration counts: no host round trip). */
int mpcmp_rh_init(mpcmp_ctx *ctx, int B, const double *x0, const double *xf);
/* Arrival.  The reference's re-solve loop has no end (the caller of solve_trajectory(false) decides, motionPlanner.cpp:199-207), and an OCP whose
 * start already lies in its terminal box degenerates (T -> lbT = 0).  After every solve the driver therefore RETIRES an instance
 *   - whose plan ends within the control period (T <= dt): it follows the plan to its last node first, or
 *   - whose advanced state lies inside the terminal box, |x - x_target|_inf <= eps_target (motionPlanner.hpp:44).
 * A retired instance keeps its state, last solution and record (status |= MPCMP_STATUS_ARRIVED) and is not re-solved: at N = 13 and N = 19 the
 * workgroups of every kernel return at once for it; at N = 25 its QP kernels (k_qp3f, k_qp3) still run on its last linearisation every SQP
 * iteration and their results are discarded (the other kernels return at once).  An instance whose solve failed hard (NaN, lost positive definiteness, dead exchange) or left the box of T holds its state and
 * re-solves from the driver's start guess with zero multipliers.
 * Start guess of the driver (first solve of every instance, and such restarts): the jerk-limited time-synchronised trajectory from the current
 * state to the target — what the reference takes from Ruckig for solve_trajectory(true), motionPlanner.cpp:146-175 — with the velocity and
 * acceleration limits of the configuration and the jerk margin of the reference's examples (0.1 x max jerk, examples/offline_trajectory.cpp:9);
 * every other re-solve re-guesses from the previous solution (solve_trajectory(false), motionPlanner.cpp:199-207).
 * Defaults of the driver: the re-solves run with carry_multipliers = 1 and qp_warm_start = 1 (a re-solve continues from the multipliers and
 * duals of the one before) unless the configuration sets a flag to -1.  mpcmp_solve_batch is unaffected (0 = off there). */
int mpcmp_rh_run(mpcmp_ctx *ctx, int steps, double dt, int use_graph);
int mpcmp_rh_get(mpcmp_ctx *ctx, double *x0_now, double *sol_x, double *sol_u, double *sol_T, mpcmp_info *info);
/* counters since mpcmp_rh_init: re-solves actually executed (instance-steps of live instances) and instances retired now (retired by a step and not
 * revived by mpcmp_rh_update since; without updates: instances retired so far); either may be NULL */
int mpcmp_rh_stats(mpcmp_ctx *ctx, long long *resolves_done, long long *arrived);
/* Feedback: the loop closed from outside, between two mpcmp_rh_run calls (MotionPlanner::set_current_state / set_target_state, then
 * solve_trajectory(false): motionPlanner.cpp:27-53,177-208).  Overwrites the current state and / or the target of n instances of the loop started by
 * mpcmp_rh_init; the update applies to the next step mpcmp_rh_run executes (eager or graph replay: the captured step stays valid).
 * idx [n]: instance indices (NULL: n == B and instance i = row i); x [n][14 narm] measured states, xf [n][14 narm] targets (either may be NULL =
 * unchanged; not both).  What the next solve of a listed instance starts from:
 *   instance before the update   given                          next solve
 *   live                         x only, no flag                re-guess from its previous solution, head := new state, tail := target, carried
 *                                                               multipliers kept (the rule of every step, fed with a measured state)
 *   live                         xf, or MPCMP_RH_RESTART        restart: the driver's start guess (jerk-limited, current state -> current target)
 *                                                               and zero multipliers, as a first or a failed solve gets
 *   retired (arrived)            anything                       revived: MPCMP_STATUS_ARRIVED leaves its record at once, mpcmp_rh_stats' `arrived`
 *                                                               drops by one, and a restart as above; the arrival rule applies again after the solve
 *   live                         new payload (mpcmp_set_payloads no restart: re-guess from its previous solution with its carried multipliers;
 *                                [_device] between two runs)    only its linearisation sees the new model (a grasp or a release mid-motion)
 *   retired (arrived)            new payload                    stays retired
 * Payload rows set between two mpcmp_rh_run calls apply to the next step, eager or graph replay.
 * An update before the first mpcmp_rh_run replaces what mpcmp_rh_init set.  mpcmp_rh_update is synchronous and returns MPCMP_EINVAL, writing
 * nothing, before mpcmp_rh_init, for n outside [1, B], an index out of range or repeated, x and xf both NULL, a value that is not finite, or an
 * unknown flag bit. */
#define MPCMP_RH_RESTART 1   /* flag: the listed instances restart from the driver's start guess even if only their state changed */
int mpcmp_rh_update(mpcmp_ctx *ctx, int n, const int *idx, const double *x, const double *xf, int flags);
/* the same with DEVICE pointers: ordered after the work already on hip_stream and before the next mpcmp_rh_run (work enqueued on hip_stream
 * afterwards waits for the update's reads of d_idx, d_x, d_xf); no host synchronisation.  The indices and values are not read on the host and not
 * checked (n, NULL pointers and flags are): an index out of range is undefined behaviour, and one listed twice takes one of its rows (a retired
 * instance is still revived and counted once). */
int mpcmp_rh_update_device(mpcmp_ctx *ctx, int n, const int *d_idx, const double *d_x, const double *d_xf, int flags, void *hip_stream);

/* ---- measurement hooks used by bench.py ---- */
/* name and accumulated device time (ms, HIP events on the solve stream) of the dominant kernel since the
 * last reset; launches = number of launches accumulated.  Event recording is OFF until the first call (a plain solve
 * records nothing and allocates nothing); afterwards at most 4096 launches are held between two calls. */
int mpcmp_kernel_timing(mpcmp_ctx *ctx, int reset, const char **name, double *ms_total, int *launches);

/* diagnostics: the first `count` doubles of one workspace array of the last solve (which: 0 iterate z, 1 multipliers, 2 collocation
 * defects c_eq, 3 path constraint values g, 4 QP step p, 5 QP duals y), in the device's internal layout */
int mpcmp_debug_fetch(mpcmp_ctx *ctx, int which, double *out, long count);

/* diagnostics: per-problem phase cycle stamps of the last k_qp launch, [B][160] (16 workgroup stamps, then
 * [16 waves][8] busy cycles per ADMM phase, then 16 stamps of the step kernel); zeros unless the library was built with -DMPCMP_STAMPS (tools/stamps.py). */
int mpcmp_debug_stamps(mpcmp_ctx *ctx, int B, unsigned long long *out);

#ifdef __cplusplus
}
#endif
#endif
