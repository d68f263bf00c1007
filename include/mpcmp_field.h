/* mpcmp_field.h — clearance against a voxel world, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model,
 * mpcmp_sphere and mpcmp_clearance, and mpcmp.h includes it where they are known. */
#ifndef MPCMP_FIELD_H
#define MPCMP_FIELD_H

/* ---- voxel worlds: an occupancy grid or a point cloud as the world, read through a Euclidean distance field built on the GPU ----
 * mpcmp_set_obstacles knows at most 256 hand-written primitives per set.  What a depth camera sees is an occupancy grid or a point cloud of 10^5 to
 * 10^7 cells that changes with every frame.  Here such a world is uploaded once per frame, turned into an exact squared distance field on the GPU,
 * and the check reads ONE field entry per (sample, robot sphere) instead of looping over obstacles.  New surface only: a checker of finished plans.
 * No solve, warm start, receding-horizon path or earlier checker reads any of it, the earlier checks stay bit for bit as they are, and mpcmp_create
 * allocates nothing for it.  The sphere tables, both arm layouts, every num_seg, the samples and the world centres are those of
 * mpcmp_clearance_batch; the record is mpcmp_clearance, so mpcmp_select_clear_batch, mpcmp_select_checked_batch and mpcmp_route_join take it as it is.
 *
 * GRID.  mpcmp_field_desc, world frame, axis-aligned: voxel (i, j, k) is the cube origin + h [i, i+1] x [j, j+1] x [k, k+1], its linear index
 *   (k n[1] + j) n[0] + i.  1 <= n[d] <= 1024, n[0] n[1] n[2] <= 2^24, h > 0 and finite, a finite origin.
 * OCCUPANCY.  unsigned char occ [n[2]][n[1]][n[0]]; nonzero: the cube is solid.  Outside the grid the world is EMPTY BY DECLARATION: a grid
 *   must cover what the robot can reach, or be merged with primitives that do (mpcmp_clearance_merge_batch).
 * FIELD.  unsigned d2 [..], the same layout: d2[v] = min over occupied w of |v - w|^2 in voxel units, (i - i')^2 + (j - j')^2 + (k - k')^2.  An
 *   exact integer, so the result does not depend on the algorithm, the launch or the device; MPCMP_FIELD_EMPTY everywhere when nothing is
 *   occupied.  The transform uses no floating point.
 * DISTANCE of a world point x:
 *   u = (x - origin) / h,   uc = clamp(u, 0, n) componentwise,   v = min(floor(uc), n - 1),   e = uc - (v + 0.5),
 *   sd_field(x) = h (sqrt((double) d2[v]) - |e| - sqrt(3)/2),   +inf on an empty field.
 *   Properties (tests/test_field_host.py pins them):
 *   - For every x, sd_field(x) is a LOWER BOUND of the distance from x to the union of the occupied cubes: every occupied centre is at least
 *     h sqrt(d2[v]) from the centre of v, x (clamped) is h |e| from that centre, and a cube reaches h sqrt(3)/2 from its own centre; clamping onto
 *     the grid box is a projection onto a convex set that contains every cube, so it cannot increase a distance to one.
 *   - For x inside the grid the bound is at most (3 sqrt(3)/2) h below the true distance (the centre of the nearest occupied voxel lies in its cube and
 *     is at most h (sqrt(d2[v]) + |e|) from x, and |e| <= sqrt(3)/2).
 *   - Inside an occupied voxel sd_field is negative (d2 = 0).  That signals a hit; it is NOT a penetration depth.
 *   - sd_field(x) <= max(sd_true(x), 0).
 *   - The true distance is 1-Lipschitz and sd_field lies below it, so a certified check may use sd_field at interval midpoints unchanged:
 *     mpcmp_clearance_certified_field_batch (mpcmp_field_cert.h) is that check, and states what its certificate means.
 * CLEARANCE of robot sphere s: sd_field(c_s) - r_s, the world centres c_s from the chain of mpcmp.h.  The record is mpcmp_clearance: `other` is
 *   the linear index of the voxel read at d_min; ties of d_min go to the lowest sample, then the lowest sphere; n_hit, t_first, status and
 *   MPCMP_CLR_NAN are as in mpcmp_clearance_batch.  With no spheres, or on an empty field, the "no pair" record of that function.
 *   The field check knows no robot pairs and no primitives: merge its records with those of mpcmp_clearance_batch (below).
 * Records do not depend on the launch or on the batch around a problem. */
typedef struct { double origin[3]; double h; int n[3]; int pad; } mpcmp_field_desc;   /* 48 bytes, world frame */
#define MPCMP_FIELD_EMPTY 0xFFFFFFFFu
#define MPCMP_FIELD_MAX_DIM 1024
#define MPCMP_FIELD_MAX_VOXELS (1 << 24)

/* ---- the rule on the host (no context, no GPU), the same source as the kernels ---- */
/* The exact transform: occ and d2 as above.  Three separable passes of a min-plus sweep, O(n) work per voxel for a line of n: meant for tests and
 * small grids, the GPU builds the large ones.  MPCMP_EINVAL, writing nothing: a NULL pointer, a desc outside the ranges above. */
int mpcmp_field_edt(const mpcmp_field_desc *desc, const unsigned char *occ, unsigned *d2);
/* *sd = sd_field(x) for x [3], *voxel (may be NULL) = the linear index of the voxel read.  MPCMP_EINVAL: a NULL desc, d2, x or sd, a bad desc, a
 * non-finite x. */
int mpcmp_field_sd(const mpcmp_field_desc *desc, const unsigned *d2, const double *x, double *sd, int *voxel);
/* Minimum field clearance of ONE configuration q [7 narm], as mpcmp_clearance_config: spheres [n_spheres[0] + ..] arm-major; *sphere / *voxel (may be
 * NULL); d_min = +inf, sphere = -1, voxel = 0 when there is no sphere or the field is empty.  MPCMP_EINVAL: the cases of mpcmp_clearance_config and
 * of mpcmp_field_sd. */
int mpcmp_clearance_field_config(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                                 const unsigned *d2, const double *q, double *d_min, int *sphere, int *voxel);

/* ---- on a context ---- */
/* Upload the occupancy occ [n[2]][n[1]][n[0]] and build the field on the GPU.  desc == NULL clears (occ is then not read).  One field per context,
 * shared by the batch.  Device memory is allocated HERE, when the grid grows (occupancy, field and one scratch array of field size), and nowhere
 * else.  The host variant is synchronous (it waits for all work of the device before it writes, as mpcmp_set_obstacles does) and rejects with
 * MPCMP_EINVAL, changing nothing: a NULL occ, a desc outside the ranges above.  The device variant is ordered on hip_stream after the work already
 * on it and before later work of the context, as mpcmp_set_obstacles_device; a check in flight on ANOTHER stream must be ordered by the caller. */
int mpcmp_set_field(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const unsigned char *occ);
int mpcmp_set_field_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const unsigned char *d_occ, void *hip_stream);
/* A point cloud: zero the occupancy, mark the voxel that contains each point of points [n_points][3] (u = (x - origin) / h with 0 <= u[d] < n[d],
 * voxel floor(u)), build.  Non-finite points and points outside the grid are skipped; n_points >= 0 (0: an empty field). */
int mpcmp_set_field_points(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *points);
int mpcmp_set_field_points_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *d_points, void *hip_stream);
/* Synchronous download of the grid in force and its field d2_out [n[2]][n[1]][n[0]] (may be NULL).  MPCMP_EINVAL when no field is set. */
int mpcmp_get_field(mpcmp_ctx *ctx, mpcmp_field_desc *desc_out, unsigned *d2_out);

/* sol_x [B][N][14 narm], sol_T [B], the n_pts + 1 uniform samples of mpcmp_clearance_batch, 1 <= n_pts <= 4096; out [B].  One workgroup per plan:
 * the forward kinematics run once per sample, then one field entry is read per (sample, sphere).  MPCMP_EINVAL, writing nothing: the cases of
 * mpcmp_clearance_batch, and no field set.  The device variant allocates nothing and makes no host round trip. */
int mpcmp_clearance_field_batch(mpcmp_ctx *ctx, int B, const double *sol_x, const double *sol_T, int n_pts, double margin, mpcmp_clearance *out);
int mpcmp_clearance_field_batch_device(mpcmp_ctx *ctx, int B, const double *d_sol_x, const double *d_sol_T, int n_pts, double margin,
                                       mpcmp_clearance *d_out, void *hip_stream);
/* One record per problem from two record arrays a [B], b [B] taken at the same n_pts and margin; typically a = the primitive world and the robot
 * pairs (mpcmp_clearance_batch), b = the field.  The rule of mpcmp_route_join: the smaller d_min among the records that have a pair, with its
 * t_min, sphere and other, ties to a; t_first the smaller non-negative one; n_hit the sum (a sample hit in both is counted in both); status the
 * OR.  Either has MPCMP_CLR_NAN: d_min = NaN, t_min = t_first = -1, sphere = -1, other = 0, n_hit = 0, status still the OR.  Neither has a pair:
 * the "no pair" record.  source [B] (may be NULL) receives 0 or 1 for where d_min came from (0 when it came from neither), because `other` alone
 * no longer says which index space it is in.  out may be a or b.  MPCMP_EINVAL, writing nothing: B < 1, a NULL a, b or out. */
int mpcmp_clearance_merge_batch(mpcmp_ctx *ctx, int B, const mpcmp_clearance *a, const mpcmp_clearance *b, mpcmp_clearance *out, int *source);
int mpcmp_clearance_merge_batch_device(mpcmp_ctx *ctx, int B, const mpcmp_clearance *d_a, const mpcmp_clearance *d_b, mpcmp_clearance *d_out,
                                       int *d_source, void *hip_stream);

#endif  /* MPCMP_FIELD_H */
