/* mpcmp_frame.h — camera frames as voxel worlds, part of include/mpcmp.h.  Include mpcmp.h, not this file: it needs mpcmp_ctx, mpcmp_model,
 * mpcmp_sphere and mpcmp_field_desc, and mpcmp.h includes it after mpcmp_field.h. */
#ifndef MPCMP_FRAME_H
#define MPCMP_FRAME_H

/* ---- frames: a point cloud, a depth image or a foreign occupancy grid turned into the voxel world of mpcmp_field.h WITHOUT the robot in it ----
 * A camera that sees the cell also sees the arm, the gripper and what the arm carries.  Marked into the occupancy those points put the robot inside
 * solid voxels at t = 0, and every plan that starts at the measured posture comes back MPCMP_CLR_HIT at its first sample.  Here the robot is
 * removed from a frame on the GPU while the frame is marked, and a depth image is unprojected there as well, so that nothing but the raw frame is
 * uploaded.  New surface only: k_field_mark, the transform and every check stay bit for bit as they are, and mpcmp_create allocates nothing for it.
 *
 * FILTER SPHERES.  The robot is the sphere tables in force (mpcmp_set_robot_spheres, up to 64 per arm, arm-major) at ONE posture q [7 narm], a HOST
 *   pointer in every variant: the encoder reading at the frame's capture time, passed to the kernel by value.  The world centres c_s are those of
 *   the chain the clearance checks run (mpcmp.h), the filter radius is R_s = r_s + pad with a finite pad >= 0.  q == NULL: no filter.  A non-NULL q
 *   with empty sphere tables filters nothing.
 * CLASS of a point x.  The tests run in this order, so every point has exactly one class:
 *   1. INVALID   a coordinate that is not finite; for a pixel also the cases of "Depth image";
 *   2. OUTSIDE   the point does not lie in the grid (u = (x - origin) / h with 0 <= u[d] < n[d] fails, as for mpcmp_set_field_points);
 *   3. ROBOT     |x - c_s|^2 <= R_s^2 for some s;
 *   4. MARKED    occ[voxel floor(u)] = 1.
 * DEPTH IMAGE.  mpcmp_camera: R (row-major) and t map the camera frame to the world frame and are used as given (R is not checked for
 *   orthogonality).  Pixel (row v, column u) holds d = depth[v * width + u], an unsigned 16-bit integer (MPCMP_DEPTH_U16) or a float
 *   (MPCMP_DEPTH_F32);  z = (double) d * depth_scale.  The pixel is INVALID when d == 0 (U16), when d is not finite or d <= 0 (F32), or when
 *   z < z_min or z > z_max (either type).  Otherwise p = (z (u - cx) / fx, z (v - cy) / fy, z) and x = R p + t, classified as a point.
 *   A valid camera: width, height >= 1, width * height <= 2^22, finite fx, fy > 0, everything else finite, depth_scale > 0, 0 <= z_min <= z_max.
 * CARVING A GRID.  For an occupancy that came from elsewhere (mpcmp_set_field, a map server): an occupied voxel is cleared when its CENTRE
 *   origin + h (i + 0.5, j + 0.5, k + 0.5) lies within R_s of some c_s, |centre - c_s|^2 <= R_s^2.
 * MPCMP_FRAME_KEEP.  The occupancy in force is not zeroed before marking: a second camera added to the first, or a camera added to a static map.
 *   It needs a field in force whose desc is identical (origin, h, n); otherwise MPCMP_EINVAL, writing nothing.
 * COUNTS.  mpcmp_frame_stats: n_in = n_invalid + n_outside + n_robot + n_marked for points and pixels (n_marked counts POINTS, not voxels);
 *   n_cleared counts carved voxels and is 0 elsewhere; a carve leaves the five point counts 0.  Integers: they do not depend on the launch.
 * GUARANTEES, for sphere centres inside the grid, from the two bounds mpcmp_field.h proves (tests/test_frame_host.py pins them):
 *   - A field built from filtered POINTS gives every sphere at the posture q a field clearance sd_field(c_s) - r_s of at least
 *     pad - (5 sqrt(3) / 2) h: a kept point lies farther than R_s from c_s, the cube it marks reaches at most h sqrt(3) closer (its diagonal), and
 *     sd_field is at most (3 sqrt(3) / 2) h below the true distance to the cubes.  (With KEEP this holds for what THIS call marks.)
 *   - After a CARVE the clearance is at least pad - 2 sqrt(3) h: a kept voxel's centre lies farther than R_s from c_s, its cube reaches at most
 *     h sqrt(3) / 2 closer, and the same bound of sd_field.
 *   - So pad > 4.34 h + margin (points, pixels) or pad > 3.47 h + margin (grids) makes the capture posture clear of the frame by construction.
 *   The other direction is a LIMITATION, not a bug: an obstacle within pad of the robot at capture time is removed with the robot. */
typedef struct { double R[9]; double t[3]; double fx, fy, cx, cy; double depth_scale; double z_min, z_max; int width, height; } mpcmp_camera;  /* 160 bytes */
typedef struct { int n_in, n_invalid, n_outside, n_robot, n_marked, n_cleared, pad[2]; } mpcmp_frame_stats;                               /* 32 bytes */
#define MPCMP_DEPTH_U16 0
#define MPCMP_DEPTH_F32 1
#define MPCMP_FRAME_KEEP 1
#define MPCMP_FRAME_MAX_PIXELS (1 << 22)

/* ---- the rule on the host (no context, no GPU), the same source as the kernels ---- */
/* The filter spheres of the posture q [7 narm]: out [n_spheres[0] + ..][4] = c_s (3), R_s.  models, narm, n_spheres and spheres as for
 * mpcmp_clearance_field_config.  MPCMP_EINVAL, writing nothing: its cases, a NULL q or out, a pad that is negative or not finite. */
int mpcmp_frame_spheres(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const double *q, double pad, double *out);
/* Mark the points [n_points][3] into occ [n[2]][n[1]][n[0]] (in-out: zeroed first unless flags has MPCMP_FRAME_KEEP) by the rule above; stats may
 * be NULL.  With q == NULL the robot arguments are not read.  With mpcmp_field_edt this is the field on the host.  MPCMP_EINVAL, writing nothing:
 * the cases of mpcmp_frame_spheres (q != NULL), a bad desc, a NULL occ, n_points < 0 or points missing, an unknown flag. */
int mpcmp_frame_points_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                           int n_points, const double *points, const double *q, double pad, int flags, unsigned char *occ, mpcmp_frame_stats *stats);
/* The same for a depth image depth [height][width] of depth_type.  MPCMP_EINVAL also: a NULL or invalid cam, a NULL depth, an unknown depth_type. */
int mpcmp_frame_depth_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                          const mpcmp_camera *cam, const void *depth, int depth_type, const double *q, double pad, int flags, unsigned char *occ,
                          mpcmp_frame_stats *stats);
/* Carve the robot out of occ (in-out); stats->n_cleared counts the voxels cleared. */
int mpcmp_frame_carve_one(const mpcmp_model *models, int narm, const int *n_spheres, const mpcmp_sphere *spheres, const mpcmp_field_desc *desc,
                          const double *q, double pad, unsigned char *occ, mpcmp_frame_stats *stats);

/* ---- on a context ---- */
/* All three mark or clear, then rebuild the field (mpcmp_set_field*): grid, allocation, ordering and the host / device variants are those of
 * mpcmp_set_field_points[_device]; the family's first use also allocates one table of 128 x 4 doubles and one counts record.  desc must not be
 * NULL here (mpcmp_set_field clears).  stats may be NULL; it is a HOST pointer in the host variants, a DEVICE pointer in the device variants, where
 * it is zeroed and written in stream order.  MPCMP_EINVAL, changing nothing: no context, a bad desc, missing data, a q with a non-finite entry, a
 * pad that is negative or not finite, an unknown flag, MPCMP_FRAME_KEEP without an identical field in force. */
/* A point cloud points [n_points][3], n_points >= 0.  With q == NULL and flags == 0 the field is bit-identical to mpcmp_set_field_points'. */
int mpcmp_set_field_points_filtered(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *points, const double *q, double pad,
                                    int flags, mpcmp_frame_stats *stats);
int mpcmp_set_field_points_filtered_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *d_points, const double *q,
                                           double pad, int flags, mpcmp_frame_stats *d_stats, void *hip_stream);
/* A depth image depth [height][width]: a host array in the host variant, a device array in the device variant.  Also MPCMP_EINVAL: an invalid
 * cam, an unknown depth_type. */
int mpcmp_set_field_depth(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const mpcmp_camera *cam, const void *depth, int depth_type, const double *q,
                          double pad, int flags, mpcmp_frame_stats *stats);
int mpcmp_set_field_depth_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const mpcmp_camera *cam, const void *d_depth, int depth_type,
                                 const double *q, double pad, int flags, mpcmp_frame_stats *d_stats, void *hip_stream);
/* Remove the robot from the occupancy in force and rebuild.  MPCMP_EINVAL when no field is set. */
int mpcmp_field_carve(mpcmp_ctx *ctx, const double *q, double pad, mpcmp_frame_stats *stats);
int mpcmp_field_carve_device(mpcmp_ctx *ctx, const double *q, double pad, mpcmp_frame_stats *d_stats, void *hip_stream);

#endif  /* MPCMP_FRAME_H */
