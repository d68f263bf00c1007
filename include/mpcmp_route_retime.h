/* mpcmp_route_retime.h — retiming of whole via-point routes, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx,
 * mpcmp_model, mpcmp_bounds, the route layout and the records of mpcmp_retime.h, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_ROUTE_RETIME_H
#define MPCMP_ROUTE_RETIME_H

/* ---- route retiming: one rate profile across the via points ----
 * mpcmp_retime_batch pins the rate to 1 at an end of a plan that is moving, and every leg of a route ends and starts moving: retimed leg by leg, a
 * route cannot slow down (or, with rate_max > 1, speed up) through a via.  But the legs of a route share position and velocity at a via, so the
 * retimed velocity lambda v is continuous across a junction exactly when lambda is: a route is ONE path with ONE profile x = lambda^2, continuous at
 * the junctions, every interval under its own leg's T, bound row and payload row.  These entry points compute that profile.  Like mpcmp_retime.h they
 * read finished trajectories only: no other entry point reads any of it, a context that never calls them behaves bit for bit as before, and
 * mpcmp_create allocates nothing for them.  Both arm layouts, every num_seg.  No jerk limits, and the acceleration still jumps at a via (as
 * mpcmp_route_seam.acc_jump_inf reports for the plan).
 *
 * EVERYTHING FOLLOWS mpcmp_retime.h (the path, the rate, the record of a grid point, its rows A w + B x + C <= 0, the caps, the A == 0 rule, the
 * elimination of w over pairs in product form, the forward step, the clock, the retimed sample) EXCEPT WHAT IS SAID HERE.
 * Layout.  The route layout of mpcmp.h: B routes, M >= 0 vias, L = B (M + 1) leg slots, leg slot l = b (M + 1) + m; sol_x [B][M+1][N][14 narm],
 * sol_u [B][M+1][N][7 narm], sol_T [L].  Bound row l and payload row l apply to leg slot l (the one rule of the row tables).
 * Grid and profile.  Each leg has n_grid intervals of its OWN normalised time: s_k = k / n_grid in leg m, Delta = 1 / n_grid.  The profile is kept
 * per leg slot, prof [L][n_grid + 1][2] = (t_k, x_k), t leg-local with t_0 = 0 in every leg, so that mpcmp_sample_retimed_batch on the L legs reads
 * it unchanged.  Point n_grid of leg m and point 0 of leg m + 1 are one state: their x is stored twice, bit for bit equal.
 * Intervals.  Interval k of leg m uses the record of point k of leg m, h = 1 / (2 T_m) and the bound and payload rows of that leg slot.
 * Pins.  The pin rule (an end at which some v_j != 0 keeps x == 1) applies only at point 0 of leg 0 and at point n_grid of leg M.  No junction is pinned.
 * Backward pass, from point n_grid of leg M down to point 0 of leg 0.  Within a leg it is that of mpcmp_retime.h.  At a junction, the set of point
 * n_grid of leg m < M is: the caps of leg m's record there and leg m's rows with A == 0 there (as for a last point: no row with w, no next-state
 * row), INTERSECTED with K_0 of leg m + 1: lo = max(lo, lo_0 of leg m + 1), hi = min(hi, hi_0 of leg m + 1).  K_0 of leg m + 1 itself is computed
 * as any K_k with k < n_grid, from leg m + 1's caps, A == 0 rows, rows with w and next-state rows.  The route is INFEASIBLE if some set is empty,
 * has hi == 0, or a pinned end lies outside its set; (leg_fail, k_fail) is the point where the backward pass met that, the highest in route order
 * (an empty intersection at a junction is reported at leg m, k_fail = n_grid; a pinned start outside its set at leg 0, k_fail = 0).
 * Forward pass.  x_0 of leg 0 = hi_0, or 1 if that start is pinned.  Within a leg as in mpcmp_retime.h.  Leg m + 1 starts from the x leg m ended
 * with: that x was clipped into leg m's last set, so it lies in K_0 of leg m + 1; hi_0 is used only at the start of leg 0.
 * Clock.  Per leg with T_m: t_0 = 0, t_k+1 = t_k + 2 T_m Delta / (sqrt(x_k) + sqrt(x_k+1)); leg_T_new [l] = t_n of that leg, and the route's
 * T_new = leg_T_new of leg 0, then + that of leg 1, .. in leg order (as mpcmp_route_join sums sol_T).  A leg clock that is not finite reports the
 * route infeasible with leg_fail = k_fail = -1.
 * Failure.  Infeasibility at any point fails the whole route.  A non-finite node value in any leg, or a sol_T of any leg that is not finite and > 0,
 * fails the whole route with MPCMP_RT_NAN (no pass is run).  A failed route has every leg's profile NaN and every leg_T_new +inf.
 * M == 0: the rule is that of mpcmp_retime_batch.
 * A record and a profile do not depend on the launch, on the route's position in the batch or on the batch around it: the passes are sequential,
 * their minima and maxima are exact, and there are no atomics.  LDS use grows neither with n_grid nor with M. */
typedef struct {
    double T_new;        /* the sum of the legs' t_n, in leg order */
    double rate_min;     /* min sqrt(x_k) over the route */
    double s_slowest;    /* the s_k of that minimum within leg_slowest; ties go to the lowest leg, then the lowest k (a junction: the earlier leg, s = 1) */
    int    leg_slowest;
    int    leg_fail;     /* -1, or the leg ... */
    int    k_fail;       /* ... and the leg-local grid point at which the backward pass failed */
    int    n_slowed;     /* number of grid points of the route with x_k < rate_max^2, a junction counted once */
    int    status;       /* MPCMP_RT_INFEASIBLE, MPCMP_RT_NAN.  With either set: T_new +inf, rate_min 0, s_slowest -1, leg_slowest -1, n_slowed 0 */
    int    pad;
} mpcmp_route_retime;    /* 48 bytes */
/* prof [L][n_grid + 1][2], leg_T_new [L] (may be NULL), out [B].  Synchronous.  MPCMP_EINVAL, writing nothing: B < 1, M < 0, L above max_batch,
 * n_grid outside [1, 4096], a required pointer NULL (spec and leg_T_new may be NULL), fewer bound rows or payload rows in force than leg slots, a
 * tool maximum that is NaN or negative, a rate_max that is not finite or <= 0, a groups bit outside MPCMP_RT_ALL_GROUPS. */
int mpcmp_retime_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid,
                             const mpcmp_retime_spec *spec, double *prof, double *leg_T_new, mpcmp_route_retime *out);
/* the arrays in DEVICE memory; spec stays a host pointer and is passed to the kernel by value.  Ordered on hip_stream, allocates nothing; checks the
 * scalars, the spec and the pointers against NULL, nothing the pointers point at */
int mpcmp_retime_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T, int n_grid,
                                    const mpcmp_retime_spec *spec, double *d_prof, double *d_leg_T_new, mpcmp_route_retime *d_out, void *hip_stream);
/* ONE route on the host (no context, no GPU), with the row, pair and clock arithmetic of the kernel: n_legs >= 1 legs x [n_legs][N][14 narm],
 * u [n_legs][N][7 narm], T [n_legs] with N = 3 num_seg + 1 (num_seg in 1 .. 8), leg m under the bounds rows[m]; models [narm] serve every leg;
 * spec may be NULL -> prof [n_legs][n_grid + 1][2], leg_T_new [n_legs] (may be NULL), out [1] */
int mpcmp_retime_route_one(const mpcmp_model *models, int narm, int num_seg, int n_legs, const mpcmp_bounds *rows, const mpcmp_retime_spec *spec,
                           const double *x, const double *u, const double *T, int n_grid, double *prof, double *leg_T_new, mpcmp_route_retime *out);
/* The retimed routes at n_pts + 1 uniform PHYSICAL times on one clock: out [B][n_pts + 1][1 + 28 narm], a row = the route time, then per arm q, qd,
 * qdd, tau (7 each); prof and n_grid as a route retime call left them.  One arm or two.  With D_m = prof [l][n_grid][0] the retimed leg durations
 * and T_new their sum in leg order, sample i is at t = (double)i / n_pts * T_new.  Its leg follows the rule of mpcmp_route_locate on the D_m: with
 * E_m the sequential prefix sums, the smallest m with t < E_m, leg M if there is none (a junction sample belongs to the later leg); the leg time is
 * t - E_m-1, kept within [0, D_m].  Inside the leg the row is the retimed-sample rule of mpcmp_retime.h at that leg time with the leg's T, profile
 * and payload row (the interval k is the largest k <= n_grid - 1 with t_k <= leg time).  Sample n_pts is leg M at s = 1.  A route with a D_m that is
 * not finite (a failed route) gets NaN rows.  MPCMP_EINVAL: B < 1, M < 0, L above max_batch, n_grid outside [1, 4096], n_pts < 1, a pointer NULL,
 * fewer payload rows than leg slots. */
int mpcmp_sample_retimed_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sol_x, const double *sol_u, const double *sol_T, int n_grid,
                                     const double *prof, int n_pts, double *out);
int mpcmp_sample_retimed_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sol_x, const double *d_sol_u, const double *d_sol_T,
                                            int n_grid, const double *d_prof, int n_pts, double *d_out, void *hip_stream);

#endif  /* MPCMP_ROUTE_RETIME_H */
