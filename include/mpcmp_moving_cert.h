/* mpcmp_moving_cert.h — certified clearance in a moving world, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx,
 * mpcmp_model, mpcmp_sphere, mpcmp_obstacle, mpcmp_clearance, mpcmp_clearance_cert and the track table of mpcmp_moving.h, and mpcmp.h includes it
 * where they are known. */
#ifndef MPCMP_MOVING_CERT_H
#define MPCMP_MOVING_CERT_H

/* ---- certified clearance in a world that moves, with the rests before and after the plan ----
 * mpcmp_clearance_certified_batch holds at every time of a plan, but in a world that stands still; mpcmp_clearance_timed_batch and
 * mpcmp_start_delay_batch know the tracks of mpcmp_set_obstacle_tracks, but only at n_pts + 1 samples, and neither looks at the robot resting at its
 * target.  This checker joins them: status == 0 means that no clearance falls below `margin` at ANY world time in
 * [t_start - wait_before, t_start + T + hold_after], the robot standing at q(0) before its motion and at q(1) after it.  New surface only: no solve,
 * warm start or earlier checker reads any of it, the earlier checks stay bit for bit as they are, and mpcmp_create allocates nothing for it.  The
 * sphere tables, the obstacle sets, the track table, both arm layouts, every num_seg, the pair set, the distance formulas and the world centres are
 * those of mpcmp_clearance_batch and mpcmp_moving.h.
 *
 * THE RULE.  Inputs per call: margin, self_gap, n_start >= 1, n_rest >= 1, 0 <= max_depth <= 16.  Per problem, each array [B] or NULL (NULL: 0):
 *   t_start[b], wait_before[b] >= 0, hold_after[b] >= 0.  There is no retime profile: the check runs on the plan's own clock.
 * Timeline.  The record clock t starts when the wait starts; w = wait_before[b], h = hold_after[b], T = sol_T[b].
 *   Wait:   the robot stands at q(0) for t in [0, w].
 *   Motion: it moves for t in [w, w + T], the normalised plan time is s = (t - w) / T.
 *   Hold:   it stands at q(1) for t in [w + T, w + T + h].
 *   World time is tau = (t_start[b] - w) + t: t_start is the world time at which the MOTION begins, as in mpcmp_clearance_timed_batch, and with
 *   w == 0 the record clock is that call's running clock.
 * Level-0 intervals, in time order: n_w = n_rest equal intervals of the wait if w > 0, else none; n_m = num_seg n_start equal intervals of the
 *   motion, exactly those of the static certificate; n_h = n_rest equal intervals of the hold if h > 0, else none; n0 = n_w + n_m + n_h <= 4096.
 *   Interval (l, i), 0 <= i < n0 2^l, lies in the level-0 interval g = i >> l and so in one phase.  With n_p the phase's level-0 count and
 *   i_p = i minus the phase's first index at level l, it covers the fraction [i_p, i_p + 1] / (n_p 2^l) of its phase; its midpoint is the exact
 *   fraction (2 i_p + 1) / (n_p 2^(l + 1)).  A fraction f of a phase is the record time f w, w + f T or (w + T) + f h.
 *   The order of midpoints across levels and phases is the integer key of the static rule, (2 i + 1) 2^(16 - l) with the GLOBAL i: below 2^29,
 *   unique and in time order.  Only the conversion from a key to a time is per phase.
 * Robot bound.  On a motion interval: dev_j, reach and D_s exactly as in mpcmp_clearance_cert.h, on the interval i_p of the n_m motion intervals.
 *   On a wait or hold interval the posture is position node 0 or node N - 1, every dev_j = 0 and D_s = 0.
 * Obstacle bound.  For track k on an interval with the world times tau_a <= tau_m <= tau_b:
 *     p_m = p_k(tau_m),   E_k = max |x - p_m|  over  x in { p_k(tau_a), p_k(tau_b) } and { P[j] : ceil(u_a) <= j <= floor(u_b) },
 *   u = clamp((tau - t0) / dt, 0, n_key - 1) the u of the track rule and |.| the Euclidean norm.  On the interval the track is a polyline with
 *   exactly those vertices, and the distance to a fixed point is convex along each piece: E_k is the exact largest displacement of the track from
 *   its midpoint offset.  A key that falls on an interval end only repeats an end point, so a last-bit difference in u between two
 *   implementations cannot change E_k by more than rounding.  n_key == 1: E_k = 0.
 * Clearances.  The midpoint clearance of sphere s against obstacle o on track k is d = sd(c_s - p_m, o) - r_s, and its bound is d - D_s - E_k (signed
 *   distance is 1-Lipschitz in the point and in the obstacle's translation); an obstacle that stands still: d - D_s; a robot pair: d - D_s - D_t.
 *   d_mid, L, the decision order (HIT, CLEAR, UNDECIDED at max_depth, else split), the capacity rule (4096 intervals per level, the first 2048 in
 *   time order are split), breadth first in time order, and the tie order of d_min and d_lower are those of the static rule.
 *
 * Records.  mpcmp_clearance and mpcmp_clearance_cert with their layouts unchanged; t_min, t_first and t_lower are on the record clock.  A non-finite
 *   position node, sol_T, t_start, wait_before or hold_after (and, for the _device call, a negative wait_before or hold_after): the MPCMP_CLR_NAN
 *   record of mpcmp_clearance_batch and the NaN certificate.
 * Consequences.  mpcmp_select_clear_batch, mpcmp_select_checked_batch and mpcmp_route_join take the records unchanged, as they take those of the
 *   static certificate.  Unlike the static certificate this one is NOT a property of the path: it holds for the plan run on its own clock from
 *   t_start and does not survive retiming or another start time.  A plan's two records do not depend on the launch or on the batch around it.
 * Out of scope: retime profiles, rotating obstacles, a certified search over all delays on the GPU, any change to a solve path. */

/* sol_x [B][N][14 narm], sol_T [B]; t_start, wait_before, hold_after [B] or NULL; out [B]; cert [B] or NULL.  Synchronous.  MPCMP_EINVAL, writing
 * nothing: what mpcmp_clearance_certified_batch refuses, n_rest < 1, num_seg n_start + 2 n_rest > 4096, a negative wait_before or hold_after
 * entry. */
int mpcmp_clearance_certified_timed_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, const double *t_start,
                                          const double *wait_before, const double *hold_after, double margin, int self_gap, int n_start, int n_rest,
                                          int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert);
/* the arrays in DEVICE memory, ordered on hip_stream: no host round trip, and nothing is allocated after a context's first call.  Their CONTENTS
 * are not looked at: a negative duration gives the NaN record */
int mpcmp_clearance_certified_timed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, const double *d_t_start,
                                                 const double *d_wait_before, const double *d_hold_after, double margin, int self_gap, int n_start,
                                                 int n_rest, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, void *hip_stream);
/* The whole rule for ONE plan x [N][14 narm] of duration T on the host (no context, no GPU), the same source as the kernel; the leading arguments
 * are those of mpcmp_clearance_timed_one (n_tracks == 0: a static world).  out [1]; cert [1] or NULL.  MPCMP_EINVAL, writing nothing: the cases of
 * mpcmp_clearance_certified_one, of mpcmp_clearance_timed_one's world and of the batch call. */
int mpcmp_clearance_certified_timed_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                        const mpcmp_obstacle *obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                                        const double *offsets, const double *x, double T, double t_start, double wait_before, double hold_after,
                                        double margin, int self_gap, int n_start, int n_rest, int max_depth, mpcmp_clearance *out,
                                        mpcmp_clearance_cert *cert);

#endif  /* MPCMP_MOVING_CERT_H */
