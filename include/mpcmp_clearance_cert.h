/* mpcmp_clearance_cert.h — certified clearance, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model,
 * mpcmp_sphere, mpcmp_obstacle and mpcmp_clearance, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_CLEARANCE_CERT_H
#define MPCMP_CLEARANCE_CERT_H

/* ---- certified clearance: an adaptive check that holds BETWEEN its evaluation points ----
 * mpcmp_clearance_batch looks at n_pts + 1 samples and says nothing about the time between them.  This checker bounds the motion of every robot
 * sphere on whole time intervals, so that status == 0 means: no clearance of the plan falls below `margin` at ANY time in [0, T]; it refines only
 * where the robot is close to something.  New surface only: no solve, warm start or other checker reads any of it, a context that never calls these
 * entry points behaves bit for bit as before, and mpcmp_create allocates nothing for them.  The sphere tables, the obstacle sets (one world or one
 * set per problem), both arm layouts, every num_seg, the pair set, the distance formulas and the world centres are those of mpcmp_clearance_batch.
 *
 * THE RULE.  Inputs per call: margin, self_gap, n_start >= 1, 0 <= max_depth <= 16.
 * Intervals.  n0 = num_seg n_start level-0 intervals, 1 <= n0 <= 4096, split the normalised time [0, 1] equally; n0 is a multiple of num_seg, so no
 *   interval of any level straddles a segment boundary and every joint position is ONE cubic on it.  Interval (l, i), 0 <= i < n0 2^l, covers
 *   [i, i + 1] h with h = 1 / (n0 2^l); its midpoint is t_m = (2 i + 1) / (n0 2^(l + 1)); its segment is floor(i / (n_start 2^l)).
 * Joint deviation.  For joint column j on an interval with the ends t_a, t_b: the Bezier control points of the cubic restricted to the interval,
 *   b0 = q(t_a),  b1 = b0 + (h / 3) q'(t_a),  b2 = b3 - (h / 3) q'(t_b),  b3 = q(t_b),
 *   q' the derivative of the position interpolant in normalised time (not the velocity channel of sol_x); all evaluations on the interval's own
 *   segment (a t_b that is a segment boundary does not fall into the next segment).  dev_j = max_k |b_k - q(t_m)|.  The cubic lies in the hull of
 *   its control points, so |q_j(t) - q_j(t_m)| <= dev_j on the interval.
 * Reach.  For sphere s on joint j_s of its arm and each joint i <= j_s: reach[s][i] = |c_s| + sum_{k = i + 1 .. j_s} |p[k]| (mpcmp_model.p), a bound
 *   of the distance from the origin of joint i to the sphere's centre in every posture.  Moving the joints one at a time,
 *   |c_s(t) - c_s(t_m)| <= D_s = sum_{i <= j_s} reach[s][i] dev_{7 a + i}  on the interval (a: the sphere's arm).
 * Bounds per pair.  Signed distance is 1-Lipschitz in the point: a sphere-obstacle pair with the midpoint clearance d has a clearance >= d - D_s on
 *   the whole interval, a robot pair (s, t) >= d - D_s - D_t.  Per interval d_mid = the smallest midpoint clearance, L = the smallest bound, both over
 *   all pairs (+inf when there is no pair).
 * Decision per interval, in this order:  d_mid < margin: a HIT leaf;  L >= margin: a CLEAR leaf;  l == max_depth: an UNDECIDED leaf;  otherwise the
 *   interval is split into (l + 1, 2 i) and (l + 1, 2 i + 1).
 * Capacity.  A level holds at most 4096 intervals (a constant of this interface).  Levels run breadth first, each in time order; if more than 2048
 *   intervals of a level are to be split, the first 2048 in time order are split and the others become UNDECIDED leaves with their own L.
 *
 * Two records per plan.  mpcmp_clearance (layout as ever): d_min = the smallest midpoint clearance evaluated (ties: lowest t_m, then lowest sphere,
 * then obstacles before robot pairs, then lowest index; distinct intervals never share a midpoint), t_min = t_m sol_T[b], sphere and other as
 * ever; t_first = the midpoint time of the earliest HIT leaf (-1 if none); n_hit = the number of HIT leaves; status = MPCMP_CLR_HIT if there is a HIT
 * leaf, ORed with MPCMP_CLR_UNDECIDED if there is an UNDECIDED leaf.  A non-finite position node: status = MPCMP_CLR_NAN alone and the fields of
 * mpcmp_clearance_batch for that case.  mpcmp_clearance_cert: below.  status == 0: the plan is certified clear at `margin`; the true minimum
 * clearance of the plan lies in [d_lower, d_min] (up to rounding).
 * Consequences.  mpcmp_select_clear_batch and mpcmp_select_checked_batch admit clr.status == 0 only, and mpcmp_route_join ORs the legs' statuses: so
 * certified records go through both unchanged, and an undecided or hit leg disqualifies its route.  The certificate is a property of the PATH: it
 * holds for the plan retimed by mpcmp_retime_batch or mpcmp_retime_route_batch too, with the times on the plan's own clock.
 * A plan's two records do not depend on the launch or on the batch around it: exact minima ordered by keys, counts, no atomics. */
#define MPCMP_CLR_UNDECIDED 4            /* status bit of mpcmp_clearance: an UNDECIDED leaf (certified calls only) */
#define MPCMP_CLR_CERT_CAPACITY 4096     /* intervals per level */
typedef struct {
    double d_lower;      /* the smallest L over all leaves: no clearance at any time of the plan is below it (+inf: no pair; NaN: a NaN plan) */
    double t_lower;      /* the midpoint time of that leaf, t_m sol_T[b]; ties go to the lowest (-1 for a NaN plan) */
    int    n_eval;       /* intervals evaluated, all levels */
    int    n_clear;      /* CLEAR leaves */
    int    n_undecided;  /* UNDECIDED leaves */
    int    depth;        /* the deepest level evaluated */
} mpcmp_clearance_cert;  /* 32 bytes; a NaN plan: the counts and depth 0 */
/* sol_x [B][N][14 narm], sol_T [B]; out [B]; cert [B] or NULL.  Synchronous.  MPCMP_EINVAL, writing nothing: what mpcmp_clearance_batch refuses
 * (B < 1, a NULL pointer other than cert, margin not finite, self_gap < 0, more problems than obstacle sets), n_start < 1, num_seg n_start > 4096,
 * max_depth outside [0, 16]. */
int mpcmp_clearance_certified_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, double margin, int self_gap, int n_start,
                                    int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert);
/* the arrays in DEVICE memory, ordered on hip_stream: no host round trip, and nothing is allocated after a context's first call */
int mpcmp_clearance_certified_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, double margin, int self_gap,
                                           int n_start, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, void *hip_stream);
/* The whole rule for ONE plan x [N][14 narm], N = 3 num_seg + 1, of duration T on the host (no context, no GPU), the same source as the kernel;
 * models, sphere tables and obstacles as for mpcmp_clearance_config.  out [1]; cert [1] or NULL.  MPCMP_EINVAL, writing nothing: the cases of
 * mpcmp_clearance_config and of the batch call, num_seg < 1. */
int mpcmp_clearance_certified_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres, int n_obs,
                                  const mpcmp_obstacle *obs, const double *x, double T, double margin, int self_gap, int n_start, int max_depth,
                                  mpcmp_clearance *out, mpcmp_clearance_cert *cert);

#endif  /* MPCMP_CLEARANCE_CERT_H */
