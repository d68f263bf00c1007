/* mpcmp_retimed_check.h — the limit checker of RETIMED plans and routes, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx,
 * mpcmp_model, mpcmp_bounds, the route layout, the records of mpcmp_limits.h and the profiles of mpcmp_retime.h / mpcmp_route_retime.h, and mpcmp.h
 * includes it where they are known. */
#ifndef MPCMP_RETIMED_CHECK_H
#define MPCMP_RETIMED_CHECK_H

/* ---- retimed plans between the grid points: the record of mpcmp_limits.h for the motion a profile stands for, and a uniform scaling of a profile ----
 * Retiming (mpcmp_retime.h, mpcmp_route_retime.h) holds its limits at the points of a grid.  The rows at grid point k bind (x_k, w_k); nothing binds
 * (x_k+1, w_k) at the right end of the interval, so where the profile turns from accelerating to braking the retimed acceleration and torque leave
 * their bounds until the next grid point.  mpcmp_limits_batch cannot see that: it reads no profile.  These entry points measure the retimed motion
 * itself and write the record mpcmp_select_checked_batch reads; with T_new as that call's sol_T the selection is on the plan the robot would run.
 * Like the other checkers they read finished data only: no solve, warm start or receding-horizon entry point reads any of it, a context that never
 * calls them behaves bit for bit as before, and mpcmp_create allocates nothing for them.  Both arm layouts, every num_seg.
 *
 * Samples.  n_pts + 1 uniform PHYSICAL times, 1 <= n_pts <= 4096: exactly the samples of mpcmp_sample_retimed_batch (for routes: of
 * mpcmp_sample_retimed_route_batch).  Sample i is at t = (double)i / n_pts * T_new; T_new is prof [b][n_grid][0] for a plan and the legs' t_n summed
 * in leg order for a route.  For a route the leg follows that sampler's rule (with E_m the sequential prefix sums of the retimed leg durations, the
 * smallest m with t < E_m, leg M if there is none: a junction sample belongs to the later leg; the leg time is t - E_m-1 kept within the leg; sample
 * n_pts is leg M at s = 1).  The interval k is the largest k <= n_grid - 1 with t_k <= t (leg time); lambda, s and w_k by the retimed-sample rule of
 * mpcmp_retime.h.
 * Values per (sample, arm):  q(s),  qd = lambda v(s),  qdd = x a(s) + (w_k / 2T) v(s),  the RNEA torque of those three with that arm's model and
 * the payload row in force (of problem b; for a route of the sample's leg slot), the tool position from q and the world-aligned tool twist J(q) qd.
 * Samples are not stored.
 * Bounds, groups and channels: mpcmp_limits.h in full: the excess rule, ties to the lowest sample, then the lowest channel, -inf for a group without
 * bounds, tol, the status bits, n_viol and t_first, the ratios and stretch = max(1, r_v, sqrt(r_a), r_lin, r_ang), all formed from the RETIMED
 * values.  The row in force is row b for a plan and the row of the sample's leg slot for a route (the configuration's tables without rows).
 * Times.  t_at and t_first are times of the retimed clock, (double)i / n_pts * T_new; for a route that is the route clock.
 * Failed profiles.  A profile whose t_n (for a route: any leg's) is not finite is a failed retime: status = MPCMP_LIM_NAN, every excess NaN, t_at -1,
 * channel -1, stretch 1, t_first -1, n_viol 0 (the record mpcmp_limits_batch writes for a non-finite sample) and T_new +inf.  A non-finite node
 * value or sol_T under a finite profile gives the same record with the finite T_new.  mpcmp_select_checked_batch rejects both.
 * A record does not depend on the launch, on the position in the batch or on the batch around it (maxima by (value, key) compares, integer sums and
 * minima, sequential leg sums; no floating-point atomics).  LDS use grows with none of n_pts, n_grid and M.
 *
 * Scaling a profile.  A uniform slow-down of a retimed motion by f > 0 is t_k *= f, x_k /= f^2: the samples stay at the same s, every retimed
 * velocity and tool twist is divided by f and every retimed acceleration by f^2.  So f = stretch of the record above makes QD, QDD, TOOL_LIN and
 * TOOL_ANG hold at the checked samples, BETWEEN ENDS AT REST; a moving end that retiming pinned to x == 1 changes its speed.  TAU, Q AND HEIGHT ARE
 * NOT CURED (the torque has a gravity part that no slowing down removes; the path stays where it is).  A factor that is not finite or <= 0 makes
 * that slot's profile NaN, and a NaN profile stays NaN.  For a route give every leg slot of the route THE SAME factor: only then does the rate stay
 * continuous at the junctions. */

/* plans: sol_x [B][N][14 narm], sol_u [B][N][7 narm], sol_T [B], prof [B][n_grid + 1][2] as mpcmp_retime_batch left it; out [B]; T_new [B] may be
 * NULL.  Synchronous.  MPCMP_EINVAL, writing nothing: B < 1 or above max_batch, n_pts outside [1, 4096], n_grid outside [1, 4096], a required
 * pointer NULL (spec and T_new may be NULL), more problems than bound rows or payload rows in force, a tol that is not finite, a tool maximum that
 * is NaN or negative. */
int mpcmp_limits_retimed_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid, const double *prof,
                               int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *out, double *T_new);
/* the arrays in DEVICE memory; spec stays a host pointer and is passed to the kernel by value.  Ordered on hip_stream, allocates nothing; checks the
 * scalars, the spec and the pointers against NULL, nothing the pointers point at */
int mpcmp_limits_retimed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_grid,
                                      const double *d_prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *d_out, double *d_T_new,
                                      void *hip_stream);
/* routes: the route layout (B routes, M vias, L = B (M + 1) leg slots), sol_T [L], prof [L][n_grid + 1][2] as mpcmp_retime_route_batch left it;
 * out [B]; T_new [B] may be NULL.  MPCMP_EINVAL as above, with M < 0, L above max_batch and fewer bound rows or payload rows in force than leg
 * slots. */
int mpcmp_limits_retimed_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid,
                                     const double *prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *out, double *T_new);
int mpcmp_limits_retimed_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T,
                                            int n_grid, const double *d_prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *d_out,
                                            double *d_T_new, void *hip_stream);
/* ONE plan (n_legs == 1) or route on the host (no context, no GPU), with the arithmetic of the kernels: n_legs >= 1 legs x [n_legs][N][14 narm],
 * u [n_legs][N][7 narm], T [n_legs] with N = 3 num_seg + 1 (num_seg in 1 .. 8), leg m under the bounds rows[m]; models [narm] serve every leg;
 * prof [n_legs][n_grid + 1][2]; spec may be NULL -> out [1], T_new [1] (may be NULL) */
int mpcmp_limits_retimed_one(const mpcmp_model *models, int narm, int num_seg, int n_legs, const mpcmp_bounds *rows, const mpcmp_limits_spec *spec,
                             const double *x, const double *u, const double *T, int n_grid, const double *prof, int n_pts, mpcmp_limits *out,
                             double *T_new);
/* prof [L][n_grid + 1][2] in place, slot l by factor [l]: t_k *= f_l, x_k /= f_l^2 (above).  Synchronous.  MPCMP_EINVAL, writing nothing: L < 1 or
 * above max_batch, n_grid outside [1, 4096], a pointer NULL. */
int mpcmp_profile_scale_batch(mpcmp_ctx *ctx, int L, int n_grid, const double *factor, double *prof);
int mpcmp_profile_scale_batch_device(mpcmp_ctx *ctx, int L, int n_grid, const double *d_factor, double *d_prof, void *hip_stream);

#endif  /* MPCMP_RETIMED_CHECK_H */
