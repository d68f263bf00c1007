/* mpcmp_field_cert.h — certified clearance against a voxel world, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx,
 * mpcmp_model, mpcmp_sphere, mpcmp_clearance, mpcmp_clearance_cert and mpcmp_field_desc, and mpcmp.h includes it after mpcmp_clearance_cert.h and
 * mpcmp_field.h, where they are known. */
#ifndef MPCMP_FIELD_CERT_H
#define MPCMP_FIELD_CERT_H

/* ---- certified clearance against a voxel world: the adaptive check of mpcmp_clearance_cert.h on the field of mpcmp_field.h ----
 * mpcmp_clearance_field_batch looks at n_pts + 1 samples and says nothing about the time between them: a pole one voxel wide passes between two
 * samples unseen.  This checker bounds the motion of every robot sphere on whole time intervals and reads the field at their midpoints, so that
 * status == 0 means "clear of the occupied cubes at EVERY time of the plan".  New surface only: no solve, warm start or earlier checker reads any
 * of it, the earlier checks stay bit for bit as they are, and mpcmp_create allocates nothing for it.  The field is the one mpcmp_set_field* put in
 * force; the sphere tables, both arm layouts, every num_seg and the world centres are those of mpcmp_clearance_batch.
 *
 * THE RULE.  Inputs per call: margin, n_start >= 1, 0 <= max_depth <= 16.  Taken UNCHANGED from mpcmp_clearance_cert.h: the intervals with
 *   n0 = num_seg n_start, the joint deviation dev_j from the Bezier control points, the reach table and D_s, the decision in its order, the
 *   capacity rule (4096 intervals per level, the first 2048 in time order are split), breadth-first levels in time order, the two records, the
 *   NaN record, and "a plan's records do not depend on the launch or on the batch around it".
 * Only the distances of an interval are new.  For sphere s at the midpoint t_m:  d_s = sd_field(c_s(t_m)) - r_s  (mpcmp_field.h, "Distance") and
 *   the bound d_s - D_s.  d_mid = the minimum of d_s over the spheres, L = the minimum of the bounds.  There are no primitives and no robot pairs:
 *   the check knows the field only, like mpcmp_clearance_field_batch.  An empty field or a robot without spheres is no special case: every distance
 *   is +inf, every level-0 interval is a CLEAR leaf, n_eval = n0, and the first record is the "no pair" record (d_min = +inf, t_min = -1,
 *   sphere = -1, other = 0) with d_lower = +inf at the first midpoint.
 * Records.  mpcmp_clearance and mpcmp_clearance_cert as in mpcmp_clearance_cert.h, except: `other` is the linear index of the voxel read at d_min
 *   (as in the sampled field check), and ties of d_min go to the lowest midpoint, then the lowest sphere; the voxel follows from those two, so it is
 *   no part of the order.
 *
 * WHAT THE CERTIFICATE MEANS.  sd_field is a LOWER BOUND of the distance to the occupied cubes, not that distance.  The true distance is
 *   1-Lipschitz in the point and sd_field lies below it, so  true(c_s(t)) >= true(c_s(t_m)) - D_s >= sd_field(c_s(t_m)) - D_s  on an interval.
 *   - status == 0: for EVERY time in [0, T] and every sphere, the distance from the sphere's centre to the union of the occupied cubes, minus r_s, is
 *     at least `margin`.
 *   - d_lower is a lower bound of that true minimum for every plan, whatever its status: every leaf's L bounds its own interval, hit and
 *     undecided leaves included.
 *   - d_min is the smallest sd_field - r seen at a midpoint.  It is NOT an upper bound of the true minimum; with that centre inside the grid, the
 *     true minimum is at most d_min + (3 sqrt(3)/2) h.
 *   - A HIT leaf is conservative by up to (3 sqrt(3)/2) h, exactly as a hit of the sampled field check is: the sphere may be that far from the
 *     cubes and still be reported.
 *   - Relation to the sampled check.  sd_field itself is not Lipschitz (it jumps at voxel faces), so a certified-clear plan may still show a hit of
 *     mpcmp_clearance_field_batch at some other instant: that hit is the conservatism of sd_field, not a clearance below the margin.  The
 *     converse is what the certificate is for: a plan the sampled check calls clear may be a certified hit.
 *   Outside the grid the world is empty by declaration (mpcmp_field.h); clamping keeps the lower-bound property there.
 *   The certificate is a property of the PATH: it holds for the plan retimed by mpcmp_retime_batch or mpcmp_retime_route_batch too, with the times on
 *   the plan's own clock.
 *
 * sol_x [B][N][14 narm], sol_T [B]; out [B]; cert [B] or NULL.  One workgroup per plan; one field entry is read per (interval, sphere).
 * MPCMP_EINVAL, writing nothing: what mpcmp_clearance_certified_batch refuses that applies here (B < 1, a NULL pointer other than cert, margin not
 * finite, n_start < 1, num_seg n_start > 4096, max_depth outside [0, 16]), and no field set.  The host variant is synchronous.  The device variant
 * is ordered on hip_stream, makes no host round trip and allocates nothing after a context's first call. */
int mpcmp_clearance_certified_field_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, double margin, int n_start, int max_depth,
                                          mpcmp_clearance *out, mpcmp_clearance_cert *cert);
int mpcmp_clearance_certified_field_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, double margin, int n_start,
                                                 int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, void *hip_stream);
/* The whole rule for ONE plan x [N][14 narm], N = 3 num_seg + 1, of duration T on the host (no context, no GPU), the same source as the kernel;
 * models and sphere tables as for mpcmp_clearance_config, desc and d2 as for mpcmp_field_sd.  out [1]; cert [1] or NULL.  MPCMP_EINVAL, writing
 * nothing: the cases of mpcmp_clearance_config and of mpcmp_field_sd that apply, those of the batch call, num_seg < 1. */
int mpcmp_clearance_certified_field_one(const mpcmp_model *models, int narm, int num_seg, const int *n_spheres, const mpcmp_sphere *spheres,
                                        const mpcmp_field_desc *desc, const unsigned *d2, const double *x, double T, double margin, int n_start,
                                        int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert);

/* CERTIFICATE MERGE.  Two mpcmp_clearance_cert arrays a [B], b [B] of the same plans become one; typically a = the primitive world and the robot
 * pairs (mpcmp_clearance_certified_batch), b = the field, at the same margin.  d_lower: the smaller of the two, ties to a, with that record's
 * t_lower;  n_eval, n_clear, n_undecided: the sums;  depth: the larger.  Either d_lower is NaN (a NaN plan): the NaN certificate (d_lower = NaN,
 * t_lower = -1, the counts and depth 0).  The merged d_lower bounds the clearance against both worlds.  The mpcmp_clearance halves of the two
 * checks go through mpcmp_clearance_merge_batch unchanged: status ORs the UNDECIDED bit as it ORs the others, and n_hit sums the HIT leaves.
 * out may be a or b.  MPCMP_EINVAL, writing nothing: B < 1, a NULL a, b or out. */
int mpcmp_clearance_cert_merge_batch(mpcmp_ctx *ctx, int B, const mpcmp_clearance_cert *a, const mpcmp_clearance_cert *b, mpcmp_clearance_cert *out);
int mpcmp_clearance_cert_merge_batch_device(mpcmp_ctx *ctx, int B, const mpcmp_clearance_cert *d_a, const mpcmp_clearance_cert *d_b,
                                            mpcmp_clearance_cert *d_out, void *hip_stream);

#endif  /* MPCMP_FIELD_CERT_H */
