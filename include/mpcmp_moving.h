/* mpcmp_moving.h — clearance against moving obstacles, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model,
 * mpcmp_sphere, mpcmp_obstacle and mpcmp_clearance, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_MOVING_H
#define MPCMP_MOVING_H

/* ---- clearance in a world that moves: tracked obstacles, a timed check, a start-delay search, a plan as another robot's world ----
 * mpcmp_clearance_batch and mpcmp_clearance_certified_batch know a world that stands still, where clearance is a property of the path.  Here
 * obstacles may translate over WORLD time, so WHEN the robot is where matters: the checks below read a retime profile and a start time together with
 * the world.  New surface only: a checker of finished plans.  No solve, warm start, receding-horizon path or earlier checker reads any of it; the
 * earlier checks never read tracks and stay bit for bit as they are, and mpcmp_create allocates nothing for it.  The sphere tables, the obstacle sets
 * (one world or one set per problem), both arm layouts, every num_seg, the pair set, the distance formulas, the world centres and the tie order are
 * those of mpcmp_clearance_batch.
 *
 * TRACKS.  A track is a translation p(tau) of an obstacle over world time tau: n_key offsets P[0 .. n_key - 1][3] on the uniform clock t0 + k dt,
 *   dt > 0, piecewise linear between keys and held constant outside them:
 *   u = clamp((tau - t0) / dt, 0, n_key - 1),  k = min(floor(u), n_key - 2),  f = u - k,  p = (1 - f) P[k] + f P[k + 1];  n_key == 1: p = P[0].
 *   A track table is offsets [n_sets][n_tracks][n_key][3] and track_of [n_sets][n_obs]: obstacle o of set i follows track track_of[i][o] of that set,
 *   -1: it stands still.  n_sets and n_obs are those of the obstacle sets in force; one (t0, dt) holds per table.  n_tracks <= 64, n_key <= 1024.
 * Clearance of robot sphere s with the world centre c_s at world time tau against obstacle o on track k:  sd(c_s - p_k(tau), o) - r_s, for every
 *   primitive type (a half-space: n.(c_s - p) - d).  Robot pairs and self_gap are as ever.
 *
 * TIMED CHECK.  Samples i = 0 .. n_pts at the plan's RUNNING time t_i = (i / n_pts) T_run.
 *   Without a profile (prof == NULL): T_run = sol_T[b], s_i = i / n_pts.
 *   With a profile [B][n_grid + 1][2] as mpcmp_retime_batch left it: T_run = t_n, and s_i is the "Retimed sample" of mpcmp_retime.h at t_i (the
 *   last sample is s = 1).
 *   q = the node interpolant of the plan at s_i; world time tau_i = t_start[b] + t_i (t_start == NULL: 0).
 *   The record is mpcmp_clearance as ever, with its tie order; t_min and t_first are on the running clock t_i.  So mpcmp_select_clear_batch,
 *   mpcmp_select_checked_batch and mpcmp_route_join take it as it is.  A profile with a non-finite entry (a plan that could not be retimed), a
 *   non-finite position node, sol_T[b] or t_start[b]: the MPCMP_CLR_NAN record of mpcmp_clearance_batch.
 *   Routes need no entry point of their own: check the leg slots as plans, each with t_start = the route's start time plus the running times of
 *   the legs before it, and join the records with mpcmp_route_join.
 *
 * START-DELAY SEARCH.  delays [K], shared by the batch: ascending, finite, >= 0, 1 <= K <= 256.  Run k of problem b is the timed check with
 *   t_start = delays[k].  With check_wait != 0 run k is joined with the robot WAITING at its start posture q(0) until it leaves: the wait is sampled
 *   at the world times delays[0 .. k], a prefix minimum over the candidate grid itself, so it sees the wait only as finely as the delays are
 *   spaced.  A run is clear when none of its samples (and wait samples) has a clearance under `margin`.
 * What happens AFTER the plan's end, with the robot resting at its target, is checked by neither call.  mpcmp_clearance_certified_timed_batch (mpcmp_moving_cert.h) checks both rests and the time between samples.
 * Records do not depend on the launch or on the batch around a problem: minima of doubles by their ordered integer keys, lowest indices, counts. */
#define MPCMP_MAX_TRACKS 64
#define MPCMP_MAX_TRACK_KEYS 1024
#define MPCMP_MAX_DELAYS 256
typedef struct {
    double delay;       /* delays[index], -1 if no run is clear */
    double d_min;       /* the smallest clearance of run `index`; no clear run: the largest of the runs' smallest clearances (NaN: a NaN plan) */
    int    index;       /* the lowest k whose run is clear, -1 if none */
    int    n_clear;     /* the number of clear runs */
    int    status;      /* 0, MPCMP_CLR_HIT (no run is clear) or MPCMP_CLR_NAN (then index -1, delay -1, n_clear 0) */
    int    pad;
} mpcmp_start_delay;    /* 32 bytes */

/* The track table of the obstacle sets in force (mpcmp_set_obstacles*): track_of [n_sets][n_obs], offsets [n_sets][n_tracks][n_key][3].
 * n_tracks == 0 removes the tracks (the other arguments are then not read), and mpcmp_set_obstacles* called afterwards makes the world static again.
 * Ordering as for mpcmp_set_obstacles: synchronous, waits for the checks in flight.  MPCMP_EINVAL, writing nothing: n_sets / n_obs that are not
 * those of the obstacle sets in force, n_tracks outside [0, 64], n_key outside [1, 1024], a track_of entry outside [-1, n_tracks), t0, dt or an
 * offset that is not finite, dt <= 0, a NULL array. */
int mpcmp_set_obstacle_tracks(mpcmp_ctx *ctx, int n_sets, int n_obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                              const double *offsets);
/* the arrays in DEVICE memory, copied on hip_stream as mpcmp_set_obstacles_device copies: their CONTENTS are not validated (a track_of entry outside
 * [-1, n_tracks) is read as -1 by the checks) */
int mpcmp_set_obstacle_tracks_device(mpcmp_ctx *ctx, int n_sets, int n_obs, const int *d_track_of, int n_tracks, int n_key, double t0, double dt,
                                     const double *d_offsets, void *hip_stream);

/* sol_x [B][N][14 narm], sol_T [B]; prof [B][n_grid + 1][2] or NULL (n_grid is then not read); t_start [B] or NULL; out [B].  Synchronous.
 * MPCMP_EINVAL, writing nothing: what mpcmp_clearance_batch refuses, and with a profile n_grid outside [1, 4096]. */
int mpcmp_clearance_timed_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, int n_grid, const double *prof,
                                const double *t_start, int n_pts, double margin, int self_gap, mpcmp_clearance *out);
/* the arrays in DEVICE memory, ordered on hip_stream: no host round trip, and nothing is allocated */
int mpcmp_clearance_timed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, int n_grid, const double *d_prof,
                                       const double *d_t_start, int n_pts, double margin, int self_gap, mpcmp_clearance *d_out, void *hip_stream);

/* delays [K]; d_min_all [B][K] or NULL: each run's smallest clearance (its wait included with check_wait; NaN for a NaN plan); out [B].
 * The forward kinematics, the obstacles that stand still and the robot pairs are evaluated once per sample, the tracked obstacles per delay.
 * MPCMP_EINVAL, writing nothing: what mpcmp_clearance_timed_batch refuses, K outside [1, 256], delays that are not finite, negative or descending. */
int mpcmp_start_delay_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, int n_grid, const double *prof, int K,
                            const double *delays, int check_wait, int n_pts, double margin, int self_gap, double *d_min_all, mpcmp_start_delay *out);
/* the arrays in DEVICE memory: the CONTENTS of d_delays are not validated (a non-finite delay gives MPCMP_CLR_NAN records) */
int mpcmp_start_delay_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, int n_grid, const double *d_prof, int K,
                                   const double *d_delays, int check_wait, int n_pts, double margin, int self_gap, double *d_min_all,
                                   mpcmp_start_delay *d_out, void *hip_stream);

/* SPHERE TRACKS OF A PLAN.  out [B][nsph][n_key][3]: the world centres of the context's robot spheres (arm-major, the numbering of
 * mpcmp_clearance.sphere) at the world times t0 + k dt.  The plan time is tau - t_start[b] clamped to [0, T_run]: the robot is held at its first
 * posture before its start and at its last posture after its end.  The layout is that of one set's track table: with nsph sphere obstacles at the
 * origin of the radii r_s and track_of = 0 .. nsph - 1, robot A's plan becomes robot B's moving world (the _device variants: no host round trip).
 * A NaN plan (as for the timed check): NaN centres.  MPCMP_EINVAL: B < 1, a NULL sol_x, sol_T or out, n_key outside [1, 1024], t0 or dt not finite,
 * dt <= 0, with a profile n_grid outside [1, 4096]. */
int mpcmp_sphere_tracks_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, int n_grid, const double *prof, const double *t_start,
                              double t0, double dt, int n_key, double *out);
int mpcmp_sphere_tracks_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, int n_grid, const double *d_prof,
                                     const double *d_t_start, double t0, double dt, int n_key, double *d_out, void *hip_stream);

/* ---- the rule on the host (no context, no GPU), the same source as the kernels ---- */
/* p [3] = the offset of the track P [n_key][3] at world time tau.  MPCMP_EINVAL: a NULL pointer, n_key outside [1, 1024], t0, dt or tau not finite,
 * dt <= 0. */
int mpcmp_track_offset(int n_key, double t0, double dt, const double *P, double tau, double *p);
/* The timed check of ONE plan x [N][14 narm], N = 3 num_seg + 1, of duration T; models, sphere tables and obstacles as for mpcmp_clearance_config;
 * track_of [n_obs] and offsets [n_tracks][n_key][3] (n_tracks == 0: a static world, neither is read); prof [n_grid + 1][2] or NULL; out [1].
 * MPCMP_EINVAL, writing nothing: the cases of mpcmp_clearance_config, of mpcmp_set_obstacle_tracks and of the batch call, num_seg < 1. */
int mpcmp_clearance_timed_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                              const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt, const double *offsets,
                              const double *x, double T, int n_grid, const double *prof, double t_start, int n_pts, double margin, int self_gap,
                              mpcmp_clearance *out);
/* ... and the start-delay search of one plan: d_min_all [K] or NULL, out [1] */
int mpcmp_start_delay_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                          const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt, const double *offsets,
                          const double *x, double T, int n_grid, const double *prof, int K, const double *delays, int check_wait, int n_pts,
                          double margin, int self_gap, double *d_min_all, mpcmp_start_delay *out);

#endif  /* MPCMP_MOVING_H */
