"""Host-side mirror of the reference's planner façade for the batched HIP path.

`Solver` is the raw context (one per GPU); `BatchMotionPlanner` keeps the member names and argument meaning
of `MotionPlanner` (mpc_solver/motionPlanner.hpp:16-176, motionPlanner.cpp) with a leading batch dimension.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import check, f64, host, lib


class Solver:
    """mpcmp_ctx wrapper. Host-buffer calls take numpy arrays; *_device calls take raw device pointers."""

    def __init__(self, cfg, max_batch, device=0, model=None, models=None):
        """models: a ctypes array of `narm` Models (multi-arm robot, mpcmp_create_multi); model: one Model; neither: the Panda"""
        self.cfg = cfg
        self.narm = len(models) if models is not None else 1
        self.nx, self.nu = 14 * self.narm, 7 * self.narm
        self.N = 3 * cfg.num_seg + 1
        self.n = 21 * self.N * self.narm + 1
        self.m = (14 * (self.N - 1) + 8 * self.N) * self.narm
        self.max_batch = int(max_batch)
        self._ctx = C.c_void_p()
        self._models = [models[a] for a in range(self.narm)] if models is not None else [model if model is not None else capi.default_model()]
        if models is not None:
            rc = lib().mpcmp_create_multi(C.byref(cfg), models, self.narm, int(device), int(max_batch), C.byref(self._ctx))
        else:
            rc = lib().mpcmp_create(C.byref(cfg), C.byref(model) if model is not None else None, int(device),
                                    int(max_batch), C.byref(self._ctx))
        check(rc)

    def close(self):
        if self._ctx:
            lib().mpcmp_destroy(self._ctx); self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg):
        check(lib().mpcmp_set_config(self._ctx, C.byref(cfg)), self._ctx); self.cfg = cfg

    # -- per-problem payloads (mpcmp_set_payloads)
    PAYLOAD_DTYPE = np.dtype([("mass", "f8"), ("com", "f8", 3), ("I", "f8", 9)])      # mpcmp_payload

    def payload_table(self, mass, com=None, inertia=None):
        """[n][narm] mpcmp_payload records from mass [n] / com [n,3] / inertia [n,3,3] (one arm) or [n,narm] / [n,narm,3] / [n,narm,3,3];
        com defaults to the model's tool point, inertia to 0"""
        mass = f64(mass)
        if self.narm == 1 and mass.ndim == 1:
            mass = mass[:, None]
        if mass.ndim != 2 or mass.shape[1] != self.narm or mass.shape[0] < 1:
            raise ValueError("mass must be [n]%s, got %s" % ("" if self.narm == 1 else "[%d]" % self.narm, mass.shape))
        n = mass.shape[0]
        lead = (n,) if self.narm == 1 else (n, self.narm)
        if com is None:
            com = np.broadcast_to(np.array([m.tool[:] for m in self._models]), (n, self.narm, 3))
        else:
            com = f64(com)
            if com.shape != lead + (3,):
                raise ValueError("com must be %s, got %s" % (list(lead + (3,)), com.shape))
        if inertia is None:
            inertia = np.zeros((n, self.narm, 3, 3))
        else:
            inertia = f64(inertia)
            if inertia.shape != lead + (3, 3):
                raise ValueError("inertia must be %s, got %s" % (list(lead + (3, 3)), inertia.shape))
        t = np.zeros((n, self.narm), dtype=self.PAYLOAD_DTYPE)
        t["mass"] = mass
        t["com"] = np.reshape(com, (n, self.narm, 3))
        t["I"] = np.reshape(inertia, (n, self.narm, 9))
        return t

    def set_payloads(self, mass, com=None, inertia=None):
        """row i applies to problem i of every later call that evaluates dynamics (include/mpcmp.h, mpcmp_set_payloads); see payload_table"""
        t = self.payload_table(mass, com, inertia)
        check(lib().mpcmp_set_payloads(self._ctx, t.shape[0], host(t)), self._ctx)
        self.payload_rows = t.shape[0]

    def clear_payloads(self):
        """back to the context's model for every problem"""
        check(lib().mpcmp_set_payloads(self._ctx, 0, None), self._ctx)
        self.payload_rows = 0

    def set_payloads_device(self, n, ptr, stream=0):
        """n rows of narm mpcmp_payload records (104 bytes each) at the device pointer ptr, ordered on `stream` (values not checked)"""
        check(lib().mpcmp_set_payloads_device(self._ctx, int(n), ptr or None, stream or None), self._ctx)
        self.payload_rows = int(n)

    # -- per-problem final-time windows, time scaling, time-synchronised solves (include/mpcmp.h)
    def set_time_windows(self, lbT, ubT):
        """row i = [lbT[i], ubT[i]] applies to problem i of every later solve, warm_start, qp and solve_synced (mpcmp_set_time_windows)"""
        lbT, ubT = f64(lbT).reshape(-1), f64(ubT).reshape(-1)
        if lbT.shape != ubT.shape or lbT.shape[0] < 1:
            raise ValueError("lbT and ubT must be [n] arrays of one length, got %s and %s" % (lbT.shape, ubT.shape))
        check(lib().mpcmp_set_time_windows(self._ctx, lbT.shape[0], host(lbT), host(ubT)), self._ctx)
        self.time_window_rows = lbT.shape[0]

    def clear_time_windows(self):
        """back to the configuration's [lbT, ubT] for every problem"""
        check(lib().mpcmp_set_time_windows(self._ctx, 0, None, None), self._ctx)
        self.time_window_rows = 0

    def set_time_windows_device(self, n, p_lb, p_ub, stream=0):
        """n rows from the device pointers p_lb / p_ub (doubles), ordered on `stream` (values not checked)"""
        check(lib().mpcmp_set_time_windows_device(self._ctx, int(n), p_lb or None, p_ub or None, stream or None), self._ctx)
        self.time_window_rows = int(n)

    # -- per-problem bounds (include/mpcmp.h, mpcmp_set_bounds)
    def bounds_table(self, n=None, margins=None, min_height=None, **tables):
        """[n] BOUNDS_DTYPE records.  Start: every row = this solver's configuration; with margins [n, 4] or [4] (position, velocity, acceleration,
        torque) row i = mpcmp_bounds_from_margins(*margins[i], min_height[i]) (min_height [n] or a scalar, default 0.05).  Then min_height
        without margins overwrites lbg[7], and explicit tables lbx / ubx [n, 14] or [14], lbu / ubu [.., 7], lbg / ubg [.., 8] overwrite theirs.
        Everything broadcasts along n; n defaults to the longest leading dimension given."""
        unknown = set(tables) - set(capi.BOUNDS_DTYPE.names)
        if unknown:
            raise ValueError("unknown bound tables %s" % sorted(unknown))
        lead = [f64(margins).shape[0]] if margins is not None and f64(margins).ndim == 2 else []
        lead += [f64(min_height).shape[0]] if min_height is not None and f64(min_height).ndim == 1 else []
        lead += [f64(v).shape[0] for v in tables.values() if f64(v).ndim == 2]
        if n is None:
            n = max(lead) if lead else 1
        n = int(n)
        if n < 1 or any(k not in (1, n) for k in lead):
            raise ValueError("bounds_table: leading dimensions %s do not broadcast to n = %d" % (lead, n))
        t = np.zeros(n, dtype=capi.BOUNDS_DTYPE)
        if margins is not None:
            mg = np.broadcast_to(f64(margins), (n, 4))
            hs = np.broadcast_to(f64(0.05 if min_height is None else min_height), (n,))
            for i in range(n):
                t[i] = capi.bounds_from_margins(mg[i, 0], mg[i, 1], mg[i, 2], mg[i, 3], hs[i])
        else:
            t[:] = capi.bounds_from_config(self.cfg)
            if min_height is not None:
                t["lbg"][:, 7] = np.broadcast_to(f64(min_height), (n,))
        for name, v in tables.items():
            t[name] = np.broadcast_to(f64(v), t[name].shape)
        return t

    def set_bounds(self, rows):
        """row i (BOUNDS_DTYPE, see bounds_table) applies to problem i of every later solve, solve_synced, qp, warm_start and pose_targets"""
        rows = np.ascontiguousarray(rows).reshape(-1)
        if rows.dtype != capi.BOUNDS_DTYPE:
            raise ValueError("rows must be an array of BOUNDS_DTYPE records")
        # (the plain address, not host(): n == 0 with NULL is the clear, and an empty table stays the error it is)
        check(lib().mpcmp_set_bounds(self._ctx, rows.shape[0], rows.ctypes.data), self._ctx)
        self.bound_rows = rows.shape[0]

    def clear_bounds(self):
        """back to the configuration's tables for every problem"""
        check(lib().mpcmp_set_bounds(self._ctx, 0, None), self._ctx)
        self.bound_rows = 0

    def set_bounds_device(self, n, ptr, stream=0):
        """n mpcmp_bounds records (464 bytes each) at the device pointer ptr, ordered on `stream` (values not checked)"""
        check(lib().mpcmp_set_bounds_device(self._ctx, int(n), ptr or None, stream or None), self._ctx)
        self.bound_rows = int(n)

    def time_scale(self, x0, xf, sx, su, sT, T_new):
        """trajectories stretched to T_new, end nodes pinned to x0 / xf (mpcmp_time_scale_batch): (ox, ou, oT)"""
        x0, xf = self._states(x0, xf)
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        T_new = f64(np.broadcast_to(np.asarray(T_new, dtype=np.float64), (B,)))
        if x0.shape[0] != B:
            raise ValueError("states are for %d problems, trajectories for %d" % (x0.shape[0], B))
        ox, ou, oT = np.zeros_like(sx), np.zeros_like(su), np.zeros(B)
        check(lib().mpcmp_time_scale_batch(self._ctx, B, host(x0), host(xf), host(sx), host(su), host(sT), host(T_new), host(ox), host(ou), host(oT)),
                                           self._ctx)
        return ox, ou, oT

    def time_scale_device(self, B, x0, xf, sx, su, sT, T_new, ox, ou, oT, stream=0):
        check(lib().mpcmp_time_scale_batch_device(self._ctx, int(B), x0 or None, xf or None, sx or None, su or None, sT or None, T_new or None,
                                                  ox or None, ou or None, oT or None, stream or None), self._ctx)

    def solve_synced(self, x0, xf, group, warm=None, n_groups=None):
        """mpcmp_solve_batch_synced: the members of each group (group[i] in [0, n_groups); -1 = on its own) that solved cleanly end at their group's
        largest final time.  Returns (sx, su, sT, info, group_T); n_groups defaults to max(group) + 1"""
        x0, xf = self._states(x0, xf); B = x0.shape[0]
        group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        if group.shape[0] != B:
            raise ValueError("group must be [B] = [%d], got %s" % (B, group.shape))
        if n_groups is None:
            n_groups = max(int(group.max()) + 1, 0)
        wx = wu = wT = None
        if warm is not None:
            wx, wu, wT = self._traj(*warm)
            if wT.shape[0] != B:
                raise ValueError("warm start is for %d problems, states for %d" % (wT.shape[0], B))
        sx, su, sT = np.zeros((B, self.N, self.nx)), np.zeros((B, self.N, self.nu)), np.zeros(B)
        info = np.zeros(B, dtype=capi.INFO_DTYPE)
        gT = np.zeros(max(n_groups, 1))
        check(lib().mpcmp_solve_batch_synced(self._ctx, B, host(x0), host(xf), host(wx), host(wu), host(wT), host(group), n_groups,
                                             host(sx), host(su), host(sT), host(info), host(gT)), self._ctx)
        return sx, su, sT, info, gT[:n_groups]

    def solve_synced_device(self, B, x0, xf, group, n_groups, sol_x, sol_u, sol_T, info=0, group_T=0, warm=(0, 0, 0), stream=0):
        check(lib().mpcmp_solve_batch_synced_device(self._ctx, int(B), x0 or None, xf or None, warm[0] or None, warm[1] or None, warm[2] or None,
                                                    group or None, int(n_groups), sol_x or None, sol_u or None, sol_T or None, info or None,
                                                    group_T or None, stream or None), self._ctx)

    # -- clearance checks: robot spheres against obstacles and against the other arm (include/mpcmp.h)
    def set_robot_spheres(self, spheres, arm=0):
        """sphere table of one arm: capi.SPHERE_DTYPE [n], n <= 64 (capi.link_spheres, capi.spheres); None or an empty table clears it"""
        t = np.zeros(0, dtype=capi.SPHERE_DTYPE) if spheres is None else capi._records(spheres, capi.SPHERE_DTYPE, "sphere").reshape(-1)
        check(lib().mpcmp_set_robot_spheres(self._ctx, int(arm), t.shape[0], host(t)), self._ctx)
        self._nsph = {**getattr(self, "_nsph", {}), int(arm): t.shape[0]}          # (sphere_tracks sizes its output by it)

    def set_obstacles(self, obstacles):
        """obstacles: capi.OBSTACLE_DTYPE [n_obs] (one world for every problem) or [n_sets][n_obs] (set i for problem i)"""
        t = capi._records(obstacles, capi.OBSTACLE_DTYPE, "obstacle")
        if t.ndim == 1:
            t = t[None, :]
        if t.ndim != 2:
            raise ValueError("obstacles must be [n_obs] or [n_sets][n_obs], got %s" % (t.shape,))
        check(lib().mpcmp_set_obstacles(self._ctx, t.shape[0], t.shape[1], host(t)), self._ctx)

    def clear_obstacles(self):
        check(lib().mpcmp_set_obstacles(self._ctx, 0, 0, None), self._ctx)

    def set_obstacles_device(self, n_sets, n_obs, ptr, stream=0):
        """[n_sets][n_obs] mpcmp_obstacle records (64 bytes each) at the device pointer ptr, ordered on `stream` (values not checked)"""
        check(lib().mpcmp_set_obstacles_device(self._ctx, int(n_sets), int(n_obs), ptr or None, stream or None), self._ctx)

    def clearance(self, sx, sT, n_pts=200, margin=0.0, self_gap=0):
        """mpcmp_clearance_batch: capi.CLEARANCE_DTYPE [B] for the trajectories sx [B][N][nx], sT [B] at n_pts + 1 uniform samples"""
        sx, sT = f64(sx), f64(sT).reshape(-1); B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d] with sT [B], got %s and %s" % (self.N, self.nx, sx.shape, sT.shape))
        out = np.zeros(B, dtype=capi.CLEARANCE_DTYPE)
        check(lib().mpcmp_clearance_batch(self._ctx, B, host(sx), host(sT), int(n_pts), float(margin), int(self_gap), host(out)), self._ctx)
        return out

    def clearance_device(self, B, sol_x, sol_T, n_pts, margin, self_gap, out, stream=0):
        check(lib().mpcmp_clearance_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, int(n_pts), float(margin), int(self_gap),
                                                 out or None, stream or None), self._ctx)

    def clearance_certified(self, sx, sT, margin=0.0, self_gap=0, n_start=4, max_depth=10):
        """mpcmp_clearance_certified_batch: (capi.CLEARANCE_DTYPE [B], capi.CLEARANCE_CERT_DTYPE [B]) for the trajectories sx [B][N][nx], sT [B]:
        status 0 means no clearance below `margin` at ANY time of the plan (include/mpcmp_clearance_cert.h)"""
        sx, sT = f64(sx), f64(sT).reshape(-1); B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d] with sT [B], got %s and %s" % (self.N, self.nx, sx.shape, sT.shape))
        out, cert = np.zeros(B, dtype=capi.CLEARANCE_DTYPE), np.zeros(B, dtype=capi.CLEARANCE_CERT_DTYPE)
        check(lib().mpcmp_clearance_certified_batch(self._ctx, B, host(sx), host(sT), float(margin), int(self_gap), int(n_start), int(max_depth),
                                                    host(out), host(cert)), self._ctx)
        return out, cert

    def clearance_certified_device(self, B, sol_x, sol_T, margin, self_gap, n_start, max_depth, out, cert=0, stream=0):
        check(lib().mpcmp_clearance_certified_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, float(margin), int(self_gap), int(n_start),
                                                           int(max_depth), out or None, cert or None, stream or None), self._ctx)

    # -- voxel worlds: an occupancy grid or a point cloud as the world, read through a distance field built on the GPU (include/mpcmp_field.h)
    def set_field(self, desc, occ=None):
        """mpcmp_set_field: desc a capi.FIELD_DESC_DTYPE record (capi.field_desc), occ [n2][n1][n0] (nonzero: solid); desc None clears"""
        if desc is None:
            check(lib().mpcmp_set_field(self._ctx, None, None), self._ctx)
            return
        desc = capi._field_desc_arg(desc)
        occ = capi._field_array(desc, np.asarray(occ) != 0, np.uint8, "occ")
        check(lib().mpcmp_set_field(self._ctx, desc.ctypes.data, host(occ)), self._ctx)

    def set_field_device(self, desc, occ, stream=0):
        """the occupancy (one byte per voxel) at the device pointer occ, ordered on `stream`; desc None clears"""
        desc = None if desc is None else capi._field_desc_arg(desc)
        check(lib().mpcmp_set_field_device(self._ctx, None if desc is None else desc.ctypes.data, occ or None, stream or None), self._ctx)

    def set_field_points(self, desc, points):
        """mpcmp_set_field_points: the voxels that contain the points [n][3] (world frame) are solid; non-finite points and points outside the
        grid are skipped"""
        desc = capi._field_desc_arg(desc); pts = f64(points).reshape(-1, 3)
        check(lib().mpcmp_set_field_points(self._ctx, desc.ctypes.data, pts.shape[0], host(pts)), self._ctx)

    def set_field_points_device(self, desc, n_points, points, stream=0):
        desc = capi._field_desc_arg(desc)
        check(lib().mpcmp_set_field_points_device(self._ctx, desc.ctypes.data, int(n_points), points or None, stream or None), self._ctx)

    def field(self, with_d2=True):
        """mpcmp_get_field: (the FIELD_DESC_DTYPE record in force, d2 [n2][n1][n0] uint32 or None)"""
        desc = np.zeros((), dtype=capi.FIELD_DESC_DTYPE)
        check(lib().mpcmp_get_field(self._ctx, desc.ctypes.data, None), self._ctx)
        if not with_d2:
            return desc, None
        n = [int(v) for v in desc["n"]]
        d2 = np.zeros((n[2], n[1], n[0]), dtype=np.uint32)
        check(lib().mpcmp_get_field(self._ctx, desc.ctypes.data, host(d2)), self._ctx)
        return desc, d2

    def clearance_field(self, sx, sT, n_pts=200, margin=0.0):
        """mpcmp_clearance_field_batch: capi.CLEARANCE_DTYPE [B] of the trajectories sx [B][N][nx], sT [B] against the field; `other` is a voxel"""
        sx, sT = f64(sx), f64(sT).reshape(-1); B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d] with sT [B], got %s and %s" % (self.N, self.nx, sx.shape, sT.shape))
        out = np.zeros(B, dtype=capi.CLEARANCE_DTYPE)
        check(lib().mpcmp_clearance_field_batch(self._ctx, B, host(sx), host(sT), int(n_pts), float(margin), host(out)), self._ctx)
        return out

    def clearance_field_device(self, B, sol_x, sol_T, n_pts, margin, out, stream=0):
        check(lib().mpcmp_clearance_field_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, int(n_pts), float(margin), out or None,
                                                       stream or None), self._ctx)

    def clearance_merge(self, a, b):
        """mpcmp_clearance_merge_batch: (one CLEARANCE_DTYPE record per problem from the records a [B] and b [B], source [B] = 0 / 1: where d_min
        came from)"""
        a = capi._records(a, capi.CLEARANCE_DTYPE, "clearance").reshape(-1); b = capi._records(b, capi.CLEARANCE_DTYPE, "clearance").reshape(-1)
        if a.shape != b.shape:
            raise ValueError("a and b must hold one record per problem each, got %s and %s" % (a.shape, b.shape))
        out, src = np.zeros(a.shape[0], dtype=capi.CLEARANCE_DTYPE), np.zeros(a.shape[0], dtype=np.int32)
        check(lib().mpcmp_clearance_merge_batch(self._ctx, a.shape[0], host(a), host(b), host(out), host(src)), self._ctx)
        return out, src

    def clearance_merge_device(self, B, a, b, out, source=0, stream=0):
        check(lib().mpcmp_clearance_merge_batch_device(self._ctx, int(B), a or None, b or None, out or None, source or None, stream or None), self._ctx)

    # -- camera frames as voxel worlds: clouds, depth images and grids with the robot removed (include/mpcmp_frame.h)
    def _frame_q(self, q):
        return None if q is None else f64(q).reshape(7 * self.narm)

    @staticmethod
    def _frame_stats(st):
        return {k: int(st[k]) for k in ("n_in", "n_invalid", "n_outside", "n_robot", "n_marked", "n_cleared")}

    def set_field_points_filtered(self, desc, points, q=None, pad=0.0, keep=False):
        """mpcmp_set_field_points_filtered: set_field_points without the points within r_s + pad of a robot sphere at the posture q [7 narm] (None:
        no filter); keep: marked into the occupancy in force.  Returns the counts as a dict"""
        desc = capi._field_desc_arg(desc); pts = f64(points).reshape(-1, 3); q = self._frame_q(q)
        st = np.zeros((), dtype=capi.FRAME_STATS_DTYPE)
        check(lib().mpcmp_set_field_points_filtered(self._ctx, desc.ctypes.data, pts.shape[0], host(pts), None if q is None else q.ctypes.data,
                                                    float(pad), capi.FRAME_KEEP if keep else 0, st.ctypes.data), self._ctx)
        return self._frame_stats(st)

    def set_field_points_filtered_device(self, desc, n_points, points, q=None, pad=0.0, keep=False, stats=0, stream=0):
        """the cloud at the device pointer `points`, the counts (32 bytes) written to the device pointer `stats` (0: none), ordered on `stream`"""
        desc = capi._field_desc_arg(desc); q = self._frame_q(q)
        check(lib().mpcmp_set_field_points_filtered_device(self._ctx, desc.ctypes.data, int(n_points), points or None, None if q is None else q.ctypes.data,
                                                           float(pad), capi.FRAME_KEEP if keep else 0, stats or None, stream or None), self._ctx)

    def set_field_depth(self, desc, camera, depth, q=None, pad=0.0, keep=False):
        """mpcmp_set_field_depth: the depth image depth [height][width] (uint16, or anything else as float32) of capi.camera(...) unprojected, filtered
        and marked on the GPU.  Returns the counts as a dict"""
        desc = capi._field_desc_arg(desc); cam = capi._camera_arg(camera); depth, kind = capi._depth_arg(cam, depth); q = self._frame_q(q)
        st = np.zeros((), dtype=capi.FRAME_STATS_DTYPE)
        check(lib().mpcmp_set_field_depth(self._ctx, desc.ctypes.data, cam.ctypes.data, depth.ctypes.data, kind, None if q is None else q.ctypes.data,
                                          float(pad), capi.FRAME_KEEP if keep else 0, st.ctypes.data), self._ctx)
        return self._frame_stats(st)

    def set_field_depth_device(self, desc, camera, depth, depth_type, q=None, pad=0.0, keep=False, stats=0, stream=0):
        desc = capi._field_desc_arg(desc); cam = capi._camera_arg(camera); q = self._frame_q(q)
        check(lib().mpcmp_set_field_depth_device(self._ctx, desc.ctypes.data, cam.ctypes.data, depth or None, int(depth_type),
                                                 None if q is None else q.ctypes.data, float(pad), capi.FRAME_KEEP if keep else 0, stats or None,
                                                 stream or None), self._ctx)

    def field_carve(self, q, pad=0.0):
        """mpcmp_field_carve: the occupied voxels whose centre lies within r_s + pad of a robot sphere at q are cleared from the occupancy in force,
        the field is rebuilt.  Returns the counts as a dict (n_cleared)"""
        q = self._frame_q(q)
        st = np.zeros((), dtype=capi.FRAME_STATS_DTYPE)
        check(lib().mpcmp_field_carve(self._ctx, None if q is None else q.ctypes.data, float(pad), st.ctypes.data), self._ctx)
        return self._frame_stats(st)

    def field_carve_device(self, q, pad=0.0, stats=0, stream=0):
        q = self._frame_q(q)
        check(lib().mpcmp_field_carve_device(self._ctx, None if q is None else q.ctypes.data, float(pad), stats or None, stream or None), self._ctx)

    # -- certified clearance against the voxel world, and the merge of two certificates (include/mpcmp_field_cert.h)
    def clearance_certified_field(self, sx, sT, margin=0.0, n_start=4, max_depth=10):
        """mpcmp_clearance_certified_field_batch: (capi.CLEARANCE_DTYPE [B], capi.CLEARANCE_CERT_DTYPE [B]) of the trajectories sx [B][N][nx], sT [B]
        against the field: status 0 means clear of the occupied cubes by `margin` at EVERY time of the plan; `other` is a voxel"""
        sx, sT = f64(sx), f64(sT).reshape(-1); B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d] with sT [B], got %s and %s" % (self.N, self.nx, sx.shape, sT.shape))
        out, cert = np.zeros(B, dtype=capi.CLEARANCE_DTYPE), np.zeros(B, dtype=capi.CLEARANCE_CERT_DTYPE)
        check(lib().mpcmp_clearance_certified_field_batch(self._ctx, B, host(sx), host(sT), float(margin), int(n_start), int(max_depth), host(out),
                                                          host(cert)), self._ctx)
        return out, cert

    def clearance_certified_field_device(self, B, sol_x, sol_T, margin, n_start, max_depth, out, cert=0, stream=0):
        check(lib().mpcmp_clearance_certified_field_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, float(margin), int(n_start),
                                                                 int(max_depth), out or None, cert or None, stream or None), self._ctx)

    def clearance_cert_merge(self, a, b, out=None):
        """mpcmp_clearance_cert_merge_batch: one CLEARANCE_CERT_DTYPE record per plan from the certificates a [B] and b [B]; out: an array to write
        into (it may be a or b), a new one by default"""
        a = capi._records(a, capi.CLEARANCE_CERT_DTYPE, "clearance_cert").reshape(-1)
        b = capi._records(b, capi.CLEARANCE_CERT_DTYPE, "clearance_cert").reshape(-1)
        if a.shape != b.shape:
            raise ValueError("a and b must hold one record per plan each, got %s and %s" % (a.shape, b.shape))
        if out is None:
            out = np.zeros(a.shape[0], dtype=capi.CLEARANCE_CERT_DTYPE)
        elif out.dtype != capi.CLEARANCE_CERT_DTYPE or out.shape != a.shape or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous CLEARANCE_CERT_DTYPE array of the shape of a")
        check(lib().mpcmp_clearance_cert_merge_batch(self._ctx, a.shape[0], host(a), host(b), host(out)), self._ctx)
        return out

    def clearance_cert_merge_device(self, B, a, b, out, stream=0):
        check(lib().mpcmp_clearance_cert_merge_batch_device(self._ctx, int(B), a or None, b or None, out or None, stream or None), self._ctx)

    # -- clearance in a moving world: tracked obstacles, timed checks, start delays, a plan as another robot's world (include/mpcmp_moving.h)
    def set_obstacle_tracks(self, track_of, offsets, t0, dt):
        """the track table of the obstacle sets in force: track_of [n_obs] or [n_sets][n_obs] (-1: the obstacle stands still), offsets
        [n_tracks][n_key][3] or [n_sets][n_tracks][n_key][3] on the clock t0 + k dt.  None / no tracks: the world stands still again"""
        if track_of is None or offsets is None or np.asarray(offsets).size == 0:
            check(lib().mpcmp_set_obstacle_tracks(self._ctx, 0, 0, None, 0, 1, 0.0, 1.0, None), self._ctx)
            return
        tof, off = np.ascontiguousarray(track_of, dtype=np.int32), f64(offsets)
        if tof.ndim == 1:
            tof = tof[None, :]
        if off.ndim == 3:
            off = off[None]
        if tof.ndim != 2 or off.ndim != 4 or off.shape[3] != 3 or off.shape[0] != tof.shape[0]:
            raise ValueError("track_of must be [n_sets][n_obs] and offsets [n_sets][n_tracks][n_key][3], got %s and %s" % (tof.shape, off.shape))
        check(lib().mpcmp_set_obstacle_tracks(self._ctx, tof.shape[0], tof.shape[1], host(tof), off.shape[1], off.shape[2], float(t0), float(dt),
                                              host(off)), self._ctx)

    def clear_obstacle_tracks(self):
        self.set_obstacle_tracks(None, None, 0.0, 1.0)

    def set_obstacle_tracks_device(self, n_sets, n_obs, track_of, n_tracks, n_key, t0, dt, offsets, stream=0):
        """the table at the device pointers track_of (int32) and offsets (float64), ordered on `stream` (values not checked)"""
        check(lib().mpcmp_set_obstacle_tracks_device(self._ctx, int(n_sets), int(n_obs), track_of or None, int(n_tracks), int(n_key), float(t0),
                                                     float(dt), offsets or None, stream or None), self._ctx)

    def _plans(self, sx, sT, prof, t_start=None):
        sx, sT = f64(sx), f64(sT).reshape(-1); B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d] with sT [B], got %s and %s" % (self.N, self.nx, sx.shape, sT.shape))
        n_grid = 0
        if prof is not None:
            prof = f64(prof)
            if prof.ndim != 3 or prof.shape[0] != B or prof.shape[2] != 2 or prof.shape[1] < 2:
                raise ValueError("prof must be [B][n_grid + 1][2], got %s" % (prof.shape,))
            n_grid = prof.shape[1] - 1
        if t_start is not None:
            t_start = f64(np.broadcast_to(np.asarray(t_start, dtype=np.float64), (B,)))
        return B, sx, sT, n_grid, prof, t_start

    def clearance_timed(self, sx, sT, prof=None, t_start=None, n_pts=200, margin=0.0, self_gap=0):
        """mpcmp_clearance_timed_batch: capi.CLEARANCE_DTYPE [B] of the plans sx, sT, run on the profiles prof [B][n_grid + 1][2] (Solver.retime) or on
        their own clock (None), started at the world times t_start (a scalar, [B] or None: 0), in the world moved by set_obstacle_tracks"""
        B, sx, sT, n_grid, prof, t_start = self._plans(sx, sT, prof, t_start)
        out = np.zeros(B, dtype=capi.CLEARANCE_DTYPE)
        check(lib().mpcmp_clearance_timed_batch(self._ctx, B, host(sx), host(sT), n_grid, host(prof), host(t_start), int(n_pts), float(margin),
                                                int(self_gap), host(out)), self._ctx)
        return out

    def clearance_timed_device(self, B, sol_x, sol_T, n_grid, prof, t_start, n_pts, margin, self_gap, out, stream=0):
        check(lib().mpcmp_clearance_timed_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, int(n_grid), prof or None, t_start or None,
                                                       int(n_pts), float(margin), int(self_gap), out or None, stream or None), self._ctx)

    def start_delay(self, sx, sT, delays, prof=None, check_wait=False, n_pts=200, margin=0.0, self_gap=0, all_minima=True):
        """mpcmp_start_delay_batch: (capi.START_DELAY_DTYPE [B], d_min_all [B][K] or None) — per plan the lowest of the candidate start delays
        [K] (ascending, >= 0) whose run has no sample under `margin`; check_wait joins each run with the wait at the start posture"""
        B, sx, sT, n_grid, prof, _ = self._plans(sx, sT, prof)
        delays = f64(delays).reshape(-1); K = delays.shape[0]
        out = np.zeros(B, dtype=capi.START_DELAY_DTYPE)
        d_all = np.zeros((B, max(K, 1))) if all_minima else None
        check(lib().mpcmp_start_delay_batch(self._ctx, B, host(sx), host(sT), n_grid, host(prof), K, host(delays), int(bool(check_wait)), int(n_pts),
                                            float(margin), int(self_gap), host(d_all), host(out)), self._ctx)
        return out, (d_all[:, :K] if all_minima else None)

    def start_delay_device(self, B, sol_x, sol_T, n_grid, prof, K, delays, check_wait, n_pts, margin, self_gap, d_min_all, out, stream=0):
        check(lib().mpcmp_start_delay_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, int(n_grid), prof or None, int(K), delays or None,
                                                   int(bool(check_wait)), int(n_pts), float(margin), int(self_gap), d_min_all or None, out or None,
                                                   stream or None), self._ctx)

    def sphere_tracks(self, sx, sT, t0, dt, n_key, prof=None, t_start=None):
        """mpcmp_sphere_tracks_batch: [B][nsph][n_key][3], the world centres of the robot spheres at the world times t0 + k dt, held at the first /
        last posture outside the plan: the layout of one set's track table"""
        B, sx, sT, n_grid, prof, t_start = self._plans(sx, sT, prof, t_start)
        nsph = sum(getattr(self, "_nsph", {}).values())
        out = np.zeros((B, nsph, int(n_key), 3))
        check(lib().mpcmp_sphere_tracks_batch(self._ctx, B, host(sx), host(sT), n_grid, host(prof), host(t_start), float(t0), float(dt), int(n_key),
                                              host(out) or host(np.zeros(1))), self._ctx)
        return out

    def sphere_tracks_device(self, B, sol_x, sol_T, n_grid, prof, t_start, t0, dt, n_key, out, stream=0):
        check(lib().mpcmp_sphere_tracks_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, int(n_grid), prof or None, t_start or None,
                                                     float(t0), float(dt), int(n_key), out or None, stream or None), self._ctx)

    # -- certified clearance in a moving world, with the rests before and after the plan (include/mpcmp_moving_cert.h)
    def clearance_certified_timed(self, sx, sT, t_start=None, wait_before=None, hold_after=None, margin=0.0, self_gap=0, n_start=4, n_rest=4,
                                  max_depth=10):
        """mpcmp_clearance_certified_timed_batch: (capi.CLEARANCE_DTYPE [B], capi.CLEARANCE_CERT_DTYPE [B]) of the plans sx, sT on their own clock in
        the world moved by set_obstacle_tracks: the motion starts at the world time t_start after a wait of wait_before at the first posture and is
        followed by a hold of hold_after at the last (each a scalar, [B] or None: 0).  status 0: no clearance below `margin` at ANY world time in
        [t_start - wait_before, t_start + T + hold_after]; times are on the record clock, which starts with the wait"""
        B, sx, sT, _, _, t_start = self._plans(sx, sT, None, t_start)
        w = None if wait_before is None else f64(np.broadcast_to(np.asarray(wait_before, dtype=np.float64), (B,)))
        h = None if hold_after is None else f64(np.broadcast_to(np.asarray(hold_after, dtype=np.float64), (B,)))
        out, cert = np.zeros(B, dtype=capi.CLEARANCE_DTYPE), np.zeros(B, dtype=capi.CLEARANCE_CERT_DTYPE)
        check(lib().mpcmp_clearance_certified_timed_batch(self._ctx, B, host(sx), host(sT), host(t_start), host(w), host(h), float(margin),
                                                          int(self_gap), int(n_start), int(n_rest), int(max_depth), host(out), host(cert)), self._ctx)
        return out, cert

    def clearance_certified_timed_device(self, B, sol_x, sol_T, t_start, wait_before, hold_after, margin, self_gap, n_start, n_rest, max_depth, out,
                                         cert=0, stream=0):
        check(lib().mpcmp_clearance_certified_timed_batch_device(self._ctx, int(B), sol_x or None, sol_T or None, t_start or None, wait_before or None,
                                                                 hold_after or None, float(margin), int(self_gap), int(n_start), int(n_rest),
                                                                 int(max_depth), out or None, cert or None, stream or None), self._ctx)

    def select_clear(self, sT, info, clr, group, n_groups=None):
        """mpcmp_select_clear_batch: per group the admissible member (clean solve status, clearance status 0) with the smallest final time,
        ties to the lowest index, -1 if none.  n_groups defaults to max(group) + 1"""
        sT = f64(sT).reshape(-1); B = sT.shape[0]
        info = np.ascontiguousarray(info); clr = np.ascontiguousarray(clr)
        group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        if info.dtype != capi.INFO_DTYPE or clr.dtype != capi.CLEARANCE_DTYPE or info.shape != (B,) or clr.shape != (B,) or group.shape != (B,):
            raise ValueError("info (INFO_DTYPE), clr (CLEARANCE_DTYPE) and group must be [B] = [%d]" % B)
        if n_groups is None:
            n_groups = max(int(group.max()) + 1, 0)
        chosen = np.full(max(int(n_groups), 1), -1, dtype=np.int32)
        check(lib().mpcmp_select_clear_batch(self._ctx, B, host(sT), host(info), host(clr), host(group), int(n_groups), host(chosen)), self._ctx)
        return chosen[:n_groups]

    def select_clear_device(self, B, sol_T, info, clr, group, n_groups, chosen, stream=0):
        check(lib().mpcmp_select_clear_batch_device(self._ctx, int(B), sol_T or None, info or None, clr or None, group or None, int(n_groups),
                                                    chosen or None, stream or None), self._ctx)

    # -- limits between the nodes (include/mpcmp.h, "limits between the nodes")
    def limits(self, sx, su, sT, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """mpcmp_limits_batch: capi.LIMITS_DTYPE [B] for the trajectories sx, su, sT at n_pts + 1 uniform samples, under the bound rows (or the
        configuration's tables) and payload rows in force.  tol: None (a NULL spec when the tool maxima are infinite too), a scalar or [7]"""
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        spec = None if tol is None and np.isposinf(tool_lin_max) and np.isposinf(tool_ang_max) else capi.limits_spec(tol, tool_lin_max, tool_ang_max)
        out = np.zeros(B, dtype=capi.LIMITS_DTYPE)
        check(lib().mpcmp_limits_batch(self._ctx, B, host(sx), host(su), host(sT), int(n_pts), None if spec is None else spec.ctypes.data,
                                       host(out)), self._ctx)
        return out

    def limits_device(self, B, sol_x, sol_u, sol_T, n_pts, out, spec=None, stream=0):
        """spec: a capi.LIMITS_SPEC_DTYPE record on the HOST (capi.limits_spec) or None; everything else raw device pointers"""
        check(lib().mpcmp_limits_batch_device(self._ctx, int(B), sol_x or None, sol_u or None, sol_T or None, int(n_pts),
                                              None if spec is None else np.ascontiguousarray(spec).ctypes.data, out or None, stream or None), self._ctx)

    # -- retiming (include/mpcmp_retime.h)
    def retime(self, sx, su, sT, n_grid=200, spec=None):
        """mpcmp_retime_batch: the time-optimal rate of every plan along its own path under the bound rows (or the configuration's tables), payload
        rows and the capi.RETIME_SPEC_DTYPE record `spec` (capi.retime_spec; None: no tool limits, never faster than the plan, all groups).
        Returns (prof [B][n_grid + 1][2] = (t_k, x_k), capi.RETIME_DTYPE [B])"""
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        spec = capi._retime_spec_arg(spec)
        prof = np.zeros((B, max(int(n_grid), 0) + 1, 2)); out = np.zeros(B, dtype=capi.RETIME_DTYPE)
        check(lib().mpcmp_retime_batch(self._ctx, B, host(sx), host(su), host(sT), int(n_grid), None if spec is None else spec.ctypes.data,
                                       host(prof), host(out)), self._ctx)
        return prof, out

    def retime_device(self, B, sol_x, sol_u, sol_T, n_grid, prof, out, spec=None, stream=0):
        """spec: a capi.RETIME_SPEC_DTYPE record on the HOST (capi.retime_spec) or None; everything else raw device pointers"""
        check(lib().mpcmp_retime_batch_device(self._ctx, int(B), sol_x or None, sol_u or None, sol_T or None, int(n_grid),
                                              None if spec is None else np.ascontiguousarray(spec).ctypes.data, prof or None, out or None,
                                              stream or None), self._ctx)

    def sample_retimed(self, sx, su, sT, prof, n_pts=200):
        """mpcmp_sample_retimed_batch: [B][n_pts + 1][1 + 28 narm] = the time i T_new / n_pts, then per arm q, qd, qdd, tau of the plans retimed by
        `prof` (what retime returned); NaN rows for a problem whose profile is NaN.  One arm or two."""
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        prof = f64(prof)
        if prof.ndim != 3 or prof.shape[0] != B or prof.shape[1] < 2 or prof.shape[2] != 2:
            raise ValueError("prof must be [B][n_grid + 1][2] = [%d][..][2]" % B)
        out = np.zeros((B, max(int(n_pts), 0) + 1, 1 + 2 * self.nx))
        check(lib().mpcmp_sample_retimed_batch(self._ctx, B, host(sx), host(su), host(sT), prof.shape[1] - 1, host(prof), int(n_pts), host(out)),
              self._ctx)
        return out

    def sample_retimed_device(self, B, sol_x, sol_u, sol_T, n_grid, prof, n_pts, out, stream=0):
        check(lib().mpcmp_sample_retimed_batch_device(self._ctx, int(B), sol_x or None, sol_u or None, sol_T or None, int(n_grid), prof or None,
                                                      int(n_pts), out or None, stream or None), self._ctx)

    # -- limits of retimed plans, profile scaling (include/mpcmp_retimed_check.h)
    def _limits_spec(self, tol, tool_lin_max, tool_ang_max):
        return None if tol is None and np.isposinf(tool_lin_max) and np.isposinf(tool_ang_max) else capi.limits_spec(tol, tool_lin_max, tool_ang_max)

    def limits_retimed(self, sx, su, sT, prof, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """mpcmp_limits_retimed_batch: (capi.LIMITS_DTYPE [B], T_new [B]) for the plans sx, su, sT retimed by `prof` (what retime returned), at the
        n_pts + 1 uniform physical times of sample_retimed, under the bound rows (or the configuration's tables) and payload rows in force.  A failed
        profile: status LIM_NAN and T_new +inf.  select_checked reads the records as they are, with T_new as its sT"""
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        prof = f64(prof)
        if prof.ndim != 3 or prof.shape[0] != B or prof.shape[2] != 2:
            raise ValueError("prof must be [B][n_grid + 1][2] = [%d][..][2]" % B)
        spec = self._limits_spec(tol, tool_lin_max, tool_ang_max)
        out = np.zeros(B, dtype=capi.LIMITS_DTYPE); T_new = np.zeros(B)
        check(lib().mpcmp_limits_retimed_batch(self._ctx, B, host(sx), host(su), host(sT), prof.shape[1] - 1, host(prof), int(n_pts),
                                               None if spec is None else spec.ctypes.data, host(out), host(T_new)), self._ctx)
        return out, T_new

    def limits_retimed_device(self, B, sol_x, sol_u, sol_T, n_grid, prof, n_pts, out, T_new=0, spec=None, stream=0):
        """spec: a capi.LIMITS_SPEC_DTYPE record on the HOST (capi.limits_spec) or None; everything else raw device pointers (0 = NULL for T_new)"""
        check(lib().mpcmp_limits_retimed_batch_device(self._ctx, int(B), sol_x or None, sol_u or None, sol_T or None, int(n_grid), prof or None,
                                                      int(n_pts), None if spec is None else np.ascontiguousarray(spec).ctypes.data, out or None,
                                                      T_new or None, stream or None), self._ctx)

    def profile_scale(self, prof, factor):
        """mpcmp_profile_scale_batch: a copy of the profiles prof [..][n_grid + 1][2] (of plans [B], or of routes [B][M + 1]) slowed uniformly,
        slot l by factor [l] (one per leading slot, in the profile's order): t_k *= f, x_k /= f^2.  f = the stretch of a limits_retimed record cures
        its QD, QDD, TOOL_LIN and TOOL_ANG groups between ends at rest.  For routes give every leg of a route the same factor (Solver.repeat)"""
        prof = np.array(f64(prof))
        if prof.ndim < 3 or prof.shape[-1] != 2 or prof.shape[-2] < 2:
            raise ValueError("prof must be [..][n_grid + 1][2]")
        L = int(np.prod(prof.shape[:-2]))
        factor = f64(factor).reshape(-1)
        if factor.shape[0] != L:
            raise ValueError("one factor per profile: %d profiles, %d factors" % (L, factor.shape[0]))
        check(lib().mpcmp_profile_scale_batch(self._ctx, L, prof.shape[-2] - 1, host(factor), host(prof)), self._ctx)
        return prof

    def profile_scale_device(self, L, n_grid, factor, prof, stream=0):
        """in place, raw device pointers"""
        check(lib().mpcmp_profile_scale_batch_device(self._ctx, int(L), int(n_grid), factor or None, prof or None, stream or None), self._ctx)

    # -- tool-line moves (include/mpcmp_toolpath.h)
    def tool_line(self, q_start, R, p, T=None, spec=None, arm=0, out=None):
        """mpcmp_tool_line_batch: straight tool lines of arm `arm` from the postures q_start [B][7] to the poses R [B][3][3], p [B][3], written as
        plans.  T [B] or a scalar: the durations (entries <= 0 and T None: the rule from the tool-speed maxima; a two-arm context needs T); spec: a
        capi.TOOL_LINE_SPEC_DTYPE record (capi.tool_line_spec) or None.  out: an existing (sx, su, sT) triple to write this arm's columns into (the
        second arm of a two-arm plan); None: new arrays, zero in the other arm's columns.  Returns (sx, su, sT, capi.TOOL_LINE_DTYPE [B])."""
        q = f64(q_start).reshape(-1, 7); B = q.shape[0]
        R, p = f64(R).reshape(B, 9), f64(p).reshape(B, 3)
        T = None if T is None else np.ascontiguousarray(np.broadcast_to(f64(T), (B,)))
        spec = capi._tool_line_spec_arg(spec)
        if out is None:
            sx, su, sT = np.zeros((B, self.N, self.nx)), np.zeros((B, self.N, self.nu)), np.zeros(B)
        else:
            sx, su, sT = out
            for a, shape in ((sx, (B, self.N, self.nx)), (su, (B, self.N, self.nu)), (sT, (B,))):
                if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shape):
                    raise ValueError("out must be C-contiguous float64 arrays of shapes (%d, %d, %d), (%d, %d, %d), (%d,)" % (B, self.N, self.nx, B, self.N, self.nu, B))
        rec = np.zeros(B, dtype=capi.TOOL_LINE_DTYPE)
        check(lib().mpcmp_tool_line_batch(self._ctx, B, int(arm), host(q), host(R), host(p), host(T), None if spec is None else spec.ctypes.data,
                                          host(sx), host(su), host(sT), host(rec)), self._ctx)
        return sx, su, sT, rec

    def tool_line_device(self, B, arm, q_start, R, p, T_in, sol_x, sol_u, sol_T, out=0, spec=None, stream=0):
        """spec: a capi.TOOL_LINE_SPEC_DTYPE record on the HOST or None; everything else raw device pointers (0 = NULL for T_in and out)"""
        check(lib().mpcmp_tool_line_batch_device(self._ctx, int(B), int(arm), q_start or None, R or None, p or None, T_in or None,
                                                 None if spec is None else np.ascontiguousarray(spec).ctypes.data, sol_x or None, sol_u or None,
                                                 sol_T or None, out or None, stream or None), self._ctx)

    def tool_deviation(self, sx, R, p, n_pts=200, tol_lin=np.inf, tol_ang=np.inf, arm=0):
        """mpcmp_tool_deviation_batch: capi.TOOL_DEV_DTYPE [B]: how far the tool of arm `arm` on the interpolant of the plans sx leaves the lines from
        the tool poses of their first nodes to R [B][3][3], p [B][3], at n_pts + 1 uniform samples.  A property of the path: it holds for the
        retimed plan too."""
        sx = f64(sx); B = sx.shape[0]
        if sx.shape != (B, self.N, self.nx):
            raise ValueError("sx must be [B][%d][%d]" % (self.N, self.nx))
        R, p = f64(R).reshape(B, 9), f64(p).reshape(B, 3)
        out = np.zeros(B, dtype=capi.TOOL_DEV_DTYPE)
        check(lib().mpcmp_tool_deviation_batch(self._ctx, B, int(arm), host(sx), host(R), host(p), int(n_pts), float(tol_lin), float(tol_ang),
                                               host(out)), self._ctx)
        return out

    def tool_deviation_device(self, B, arm, sol_x, R, p, n_pts, tol_lin, tol_ang, out, stream=0):
        check(lib().mpcmp_tool_deviation_batch_device(self._ctx, int(B), int(arm), sol_x or None, R or None, p or None, int(n_pts), float(tol_lin),
                                                      float(tol_ang), out or None, stream or None), self._ctx)

    def select_checked(self, sT, info, group, clr=None, lim=None, lim_mask=0x7F, n_groups=None):
        """mpcmp_select_checked_batch: select_clear with an optional clearance test (clr None: none) and an optional limits test (a member whose
        lim status has a bit of lim_mask, or LIM_NAN, is inadmissible).  n_groups defaults to max(group) + 1"""
        sT = f64(sT).reshape(-1); B = sT.shape[0]
        info = np.ascontiguousarray(info)
        clr = None if clr is None else np.ascontiguousarray(clr)
        lim = None if lim is None else np.ascontiguousarray(lim)
        group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        if info.dtype != capi.INFO_DTYPE or info.shape != (B,) or group.shape != (B,) or \
                (clr is not None and (clr.dtype != capi.CLEARANCE_DTYPE or clr.shape != (B,))) or \
                (lim is not None and (lim.dtype != capi.LIMITS_DTYPE or lim.shape != (B,))):
            raise ValueError("info (INFO_DTYPE), clr (CLEARANCE_DTYPE or None), lim (LIMITS_DTYPE or None) and group must be [B] = [%d]" % B)
        if n_groups is None:
            n_groups = max(int(group.max()) + 1, 0)
        chosen = np.full(max(int(n_groups), 1), -1, dtype=np.int32)
        check(lib().mpcmp_select_checked_batch(self._ctx, B, host(sT), host(info), host(clr), host(lim), int(lim_mask), host(group), int(n_groups),
                                               host(chosen)), self._ctx)
        return chosen[:n_groups]

    def select_checked_device(self, B, sol_T, info, clr, lim, lim_mask, group, n_groups, chosen, stream=0):
        check(lib().mpcmp_select_checked_batch_device(self._ctx, int(B), sol_T or None, info or None, clr or None, lim or None, int(lim_mask),
                                                      group or None, int(n_groups), chosen or None, stream or None), self._ctx)

    # -- via-point routes: B routes with M vias = B (M + 1) leg slots (include/mpcmp.h, "via-point routes")
    @staticmethod
    def repeat(rows, M):
        """one row per route -> one row per leg slot: every row M + 1 times (a route under its own payload, window or limits sets its row for each
        of its legs); works on the arrays set_payloads / set_time_windows take and on BOUNDS_DTYPE / OBSTACLE_DTYPE tables"""
        return np.ascontiguousarray(np.repeat(np.asarray(rows), int(M) + 1, axis=0))

    def _route_in(self, x0, via, via_qd, speed, xf):
        x0, xf = self._states(x0, xf); B = x0.shape[0]; nq = self.nu
        via = np.zeros((B, 0, nq)) if via is None else f64(via)
        if via.ndim != 3 or via.shape[0] != B or via.shape[2] != nq:
            raise ValueError("via must be [B][M][%d] with B = %d, got %s" % (nq, B, via.shape))
        M = via.shape[1]
        if via_qd is not None:
            via_qd = f64(via_qd)
            if via_qd.shape != via.shape:
                raise ValueError("via_qd must have the shape of via %s, got %s" % (via.shape, via_qd.shape))
        if speed is not None:
            speed = f64(np.broadcast_to(np.asarray(speed, dtype=np.float64), (B,)))
        return x0, via, via_qd, speed, xf, B, M

    def route_legs(self, x0, via, xf, via_qd=None, speed=None):
        """mpcmp_route_legs: (leg_x0 [B (M+1)][nx], leg_xf, via_qd [B][M][7 narm]); via_qd None = the chord rule at `speed` (None = 1)"""
        x0, via, via_qd, speed, xf, B, M = self._route_in(x0, via, via_qd, speed, xf)
        L = B * (M + 1)
        l0, lf, vo = np.zeros((L, self.nx)), np.zeros((L, self.nx)), np.zeros_like(via)
        check(lib().mpcmp_route_legs(self._ctx, B, M, host(x0), host(via), host(via_qd), host(speed), host(xf), host(l0), host(lf), host(vo)),
                                     self._ctx)
        return l0, lf, vo

    def route_legs_device(self, B, M, x0, via, xf, leg_x0, leg_xf, via_qd=0, speed=0, via_qd_out=0, stream=0):
        check(lib().mpcmp_route_legs_device(self._ctx, int(B), int(M), x0 or None, via or None, via_qd or None, speed or None, xf or None,
                                            leg_x0 or None, leg_xf or None, via_qd_out or None, stream or None), self._ctx)

    def solve_route(self, x0, via, xf, via_qd=None, speed=None, jmax=None):
        """mpcmp_solve_route_batch: a dict with the legs' sol_x [B][M+1][N][nx], sol_u, sol_T [B][M+1], info [B][M+1] and the routes' route_T [B],
        route_info [B] (INFO_DTYPE), seam [B] (ROUTE_SEAM_DTYPE), via_qd [B][M][7 narm].  jmax [7]: the legs start from the jerk-limited guess;
        None: from the built-in initialiser"""
        x0, via, via_qd, speed, xf, B, M = self._route_in(x0, via, via_qd, speed, xf)
        jm = None if jmax is None else f64(jmax).reshape(7)
        sx, su, sT = np.zeros((B, M + 1, self.N, self.nx)), np.zeros((B, M + 1, self.N, self.nu)), np.zeros((B, M + 1))
        info, rinfo = np.zeros((B, M + 1), dtype=capi.INFO_DTYPE), np.zeros(B, dtype=capi.INFO_DTYPE)
        rT, seam, vo = np.zeros(B), np.zeros(B, dtype=capi.ROUTE_SEAM_DTYPE), np.zeros_like(via)
        check(lib().mpcmp_solve_route_batch(self._ctx, B, M, host(x0), host(via), host(via_qd), host(speed), host(xf), host(jm),
                                            host(sx), host(su), host(sT), host(info), host(rT), host(rinfo), host(seam), host(vo)), self._ctx)
        return dict(sol_x=sx, sol_u=su, sol_T=sT, info=info, route_T=rT, route_info=rinfo, seam=seam, via_qd=vo)

    def solve_route_device(self, B, M, x0, via, xf, sol_x, sol_u, sol_T, route_T, route_info, seam, info=0, via_qd=0, speed=0, jmax=None, via_qd_out=0,
                           stream=0):
        jm = None if jmax is None else f64(jmax).reshape(7)
        check(lib().mpcmp_solve_route_batch_device(self._ctx, int(B), int(M), x0 or None, via or None, via_qd or None, speed or None, xf or None,
                                                   host(jm), sol_x or None, sol_u or None, sol_T or None, info or None, route_T or None,
                                                   route_info or None, seam or None, via_qd_out or None, stream or None), self._ctx)

    def _route_traj(self, sx, su, sT):
        sx, su, sT = f64(sx), f64(su), f64(sT)
        if sT.ndim != 2 or sx.shape != sT.shape + (self.N, self.nx) or su.shape != sT.shape + (self.N, self.nu):
            raise ValueError("route trajectories must be [B][M+1][%d][%d], [B][M+1][%d][%d], [B][M+1]; got %s, %s, %s"
                             % (self.N, self.nx, self.N, self.nu, sx.shape, su.shape, sT.shape))
        return sx, su, sT, sT.shape[0], sT.shape[1] - 1

    def route_join(self, sx, su, sT, info, clr=None):
        """mpcmp_route_join: (route_T [B], route_info [B], seam [B]) and, with the legs' clearance records clr [B][M+1], route_clr [B]"""
        sx, su, sT, B, M = self._route_traj(sx, su, sT)
        info = np.ascontiguousarray(info)
        if info.dtype != capi.INFO_DTYPE or info.shape != sT.shape:
            raise ValueError("info must be INFO_DTYPE [B][M+1]")
        rclr = None
        if clr is not None:
            clr = np.ascontiguousarray(clr)
            if clr.dtype != capi.CLEARANCE_DTYPE or clr.shape != sT.shape:
                raise ValueError("clr must be CLEARANCE_DTYPE [B][M+1]")
            rclr = np.zeros(B, dtype=capi.CLEARANCE_DTYPE)
        rT, rinfo, seam = np.zeros(B), np.zeros(B, dtype=capi.INFO_DTYPE), np.zeros(B, dtype=capi.ROUTE_SEAM_DTYPE)
        check(lib().mpcmp_route_join(self._ctx, B, M, host(sx), host(su), host(sT), host(info), host(clr), host(rT), host(rinfo), host(seam),
                                     host(rclr)), self._ctx)
        return (rT, rinfo, seam) if clr is None else (rT, rinfo, seam, rclr)

    def route_join_device(self, B, M, sol_x, sol_u, sol_T, info, route_T, route_info, seam, clr=0, route_clr=0, stream=0):
        check(lib().mpcmp_route_join_device(self._ctx, int(B), int(M), sol_x or None, sol_u or None, sol_T or None, info or None, clr or None,
                                            route_T or None, route_info or None, seam or None, route_clr or None, stream or None), self._ctx)

    def sample_route(self, sx, su, sT, n_pts=200):
        """mpcmp_sample_route_batch: out [B][n_pts+1][29] = route time, q, qd, qdd, tau on a uniform clock across the junctions"""
        sx, su, sT, B, M = self._route_traj(sx, su, sT)
        out = np.zeros((B, n_pts + 1, 29))
        check(lib().mpcmp_sample_route_batch(self._ctx, B, M, host(sx), host(su), host(sT), int(n_pts), host(out)), self._ctx)
        return out

    def sample_route_device(self, B, M, sol_x, sol_u, sol_T, n_pts, out, stream=0):
        check(lib().mpcmp_sample_route_batch_device(self._ctx, int(B), int(M), sol_x or None, sol_u or None, sol_T or None, int(n_pts), out or None,
                                                    stream or None), self._ctx)

    # -- route retiming (include/mpcmp_route_retime.h)
    def retime_route(self, sx, su, sT, n_grid=200, spec=None):
        """mpcmp_retime_route_batch: ONE rate profile per route across its via points, for the [B][M+1][..] arrays solve_route returns, under the
        bound and payload rows of the leg slots and the capi.RETIME_SPEC_DTYPE record `spec` (None: no tool limits, never faster than the plan, all
        groups).  Returns (prof [B][M+1][n_grid + 1][2] = (t_k, x_k) with leg times, leg_T_new [B][M+1], capi.ROUTE_RETIME_DTYPE [B])"""
        sx, su, sT, B, M = self._route_traj(sx, su, sT)
        spec = capi._retime_spec_arg(spec)
        prof, leg_T = np.zeros((B, M + 1, max(int(n_grid), 0) + 1, 2)), np.zeros((B, M + 1))
        out = np.zeros(B, dtype=capi.ROUTE_RETIME_DTYPE)
        check(lib().mpcmp_retime_route_batch(self._ctx, B, M, host(sx), host(su), host(sT), int(n_grid), None if spec is None else spec.ctypes.data,
                                             host(prof), host(leg_T), host(out)), self._ctx)
        return prof, leg_T, out

    def retime_route_device(self, B, M, sol_x, sol_u, sol_T, n_grid, prof, out, leg_T_new=0, spec=None, stream=0):
        """spec: a capi.RETIME_SPEC_DTYPE record on the HOST (capi.retime_spec) or None; everything else raw device pointers (0 = NULL for leg_T_new)"""
        check(lib().mpcmp_retime_route_batch_device(self._ctx, int(B), int(M), sol_x or None, sol_u or None, sol_T or None, int(n_grid),
                                                    None if spec is None else np.ascontiguousarray(spec).ctypes.data, prof or None,
                                                    leg_T_new or None, out or None, stream or None), self._ctx)

    def sample_retimed_route(self, sx, su, sT, prof, n_pts=200):
        """mpcmp_sample_retimed_route_batch: [B][n_pts + 1][1 + 28 narm] = the route time i T_new / n_pts, then per arm q, qd, qdd, tau of the routes
        retimed by `prof` (what retime_route returned), on one clock across the junctions; NaN rows for a failed route.  One arm or two."""
        sx, su, sT, B, M = self._route_traj(sx, su, sT)
        prof = f64(prof)
        if prof.ndim != 4 or prof.shape[:2] != (B, M + 1) or prof.shape[2] < 2 or prof.shape[3] != 2:
            raise ValueError("prof must be [B][M+1][n_grid + 1][2] = [%d][%d][..][2]" % (B, M + 1))
        out = np.zeros((B, max(int(n_pts), 0) + 1, 1 + 2 * self.nx))
        check(lib().mpcmp_sample_retimed_route_batch(self._ctx, B, M, host(sx), host(su), host(sT), prof.shape[2] - 1, host(prof), int(n_pts),
                                                     host(out)), self._ctx)
        return out

    def sample_retimed_route_device(self, B, M, sol_x, sol_u, sol_T, n_grid, prof, n_pts, out, stream=0):
        check(lib().mpcmp_sample_retimed_route_batch_device(self._ctx, int(B), int(M), sol_x or None, sol_u or None, sol_T or None, int(n_grid),
                                                            prof or None, int(n_pts), out or None, stream or None), self._ctx)

    def limits_retimed_route(self, sx, su, sT, prof, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """mpcmp_limits_retimed_route_batch: (capi.LIMITS_DTYPE [B], T_new [B]) for the routes sx, su, sT [B][M+1][..] retimed by `prof` (what
        retime_route returned), at the n_pts + 1 uniform times of sample_retimed_route on the route clock, every sample under the bound and payload
        rows of its leg slot.  A failed route: status LIM_NAN and T_new +inf"""
        sx, su, sT, B, M = self._route_traj(sx, su, sT)
        prof = f64(prof)
        if prof.ndim != 4 or prof.shape[:2] != (B, M + 1) or prof.shape[3] != 2:
            raise ValueError("prof must be [B][M+1][n_grid + 1][2] = [%d][%d][..][2]" % (B, M + 1))
        spec = self._limits_spec(tol, tool_lin_max, tool_ang_max)
        out = np.zeros(B, dtype=capi.LIMITS_DTYPE); T_new = np.zeros(B)
        check(lib().mpcmp_limits_retimed_route_batch(self._ctx, B, M, host(sx), host(su), host(sT), prof.shape[2] - 1, host(prof), int(n_pts),
                                                     None if spec is None else spec.ctypes.data, host(out), host(T_new)), self._ctx)
        return out, T_new

    def limits_retimed_route_device(self, B, M, sol_x, sol_u, sol_T, n_grid, prof, n_pts, out, T_new=0, spec=None, stream=0):
        """spec: a capi.LIMITS_SPEC_DTYPE record on the HOST (capi.limits_spec) or None; everything else raw device pointers (0 = NULL for T_new)"""
        check(lib().mpcmp_limits_retimed_route_batch_device(self._ctx, int(B), int(M), sol_x or None, sol_u or None, sol_T or None, int(n_grid),
                                                            prof or None, int(n_pts), None if spec is None else np.ascontiguousarray(spec).ctypes.data,
                                                            out or None, T_new or None, stream or None), self._ctx)

    def _states(self, x0, xf):
        """(x0, xf) as contiguous [B][14] arrays; a shape mismatch raises instead of letting the C side read out of bounds"""
        x0, xf = f64(x0), f64(xf)
        if x0.ndim != 2 or x0.shape[1] != self.nx or xf.shape != x0.shape:
            raise ValueError("x0 and xf must both be [B][%d] arrays, got %s and %s" % (self.nx, x0.shape, xf.shape))
        return x0, xf

    def _traj(self, sx, su, sT):
        sx, su, sT = f64(sx), f64(su), f64(sT).reshape(-1)
        B = sT.shape[0]
        if sx.shape != (B, self.N, self.nx) or su.shape != (B, self.N, self.nu):
            raise ValueError("trajectory arrays must be [B][%d][%d], [B][%d][%d], [B]; got %s, %s, %s"
                             % (self.N, self.nx, self.N, self.nu, sx.shape, su.shape, sT.shape))
        return sx, su, sT

    # -- hot path, host buffers
    def solve(self, x0, xf, warm=None):
        x0, xf = self._states(x0, xf); B = x0.shape[0]
        wx = wu = wT = None
        if warm is not None:
            wx, wu, wT = self._traj(*warm)
            if wT.shape[0] != B:
                raise ValueError("warm start is for %d problems, states for %d" % (wT.shape[0], B))
        sx, su, sT = np.zeros((B, self.N, self.nx)), np.zeros((B, self.N, self.nu)), np.zeros(B)
        info = np.zeros(B, dtype=capi.INFO_DTYPE)
        check(lib().mpcmp_solve_batch(self._ctx, B, host(x0), host(xf), host(wx), host(wu), host(wT), host(sx), host(su), host(sT), host(info)),
                                      self._ctx)
        return sx, su, sT, info

    # -- hot path, device-resident buffers (raw pointers, e.g. torch tensors' data_ptr())
    def solve_device(self, B, x0, xf, sol_x, sol_u, sol_T, info=0, warm=(0, 0, 0), stream=0):
        check(lib().mpcmp_solve_batch_device(self._ctx, int(B), x0 or None, xf or None, warm[0] or None, warm[1] or None, warm[2] or None,
                                             sol_x or None, sol_u or None, sol_T or None, info or None, stream or None), self._ctx)

    def warm_start(self, x0, xf):
        x0, xf = self._states(x0, xf); B = x0.shape[0]
        wx, wu, wT = np.zeros((B, self.N, 14)), np.zeros((B, self.N, 7)), np.zeros(B)
        check(lib().mpcmp_warm_start_batch(self._ctx, B, host(x0), host(xf), host(wx), host(wu), host(wT)), self._ctx)
        return wx, wu, wT

    def _acc(self, a, B):
        return None if a is None else f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (B, 7)))

    @staticmethod
    def _lim(v):
        return None if v is None else f64(v).reshape(7)

    def warm_start_jerk(self, x0, xf, jmax, acc0=None, accT=None, vmax=None, amax=None):
        """Jerk-limited, time-synchronised warm start (stands in for Ruckig): (warm_x [B][N][14], warm_u [B][N][7], warm_T [B]).
        acc0 / accT: boundary accelerations [B][7] (None = zero), as set_current_state / set_target_state forward them (motionPlanner.cpp:36-38,50-52).
        vmax / amax [7]: the generator's velocity / acceleration limits (None = the context's margin-applied bounds): ruckig's input.max_velocity / max_acceleration."""
        (x0, xf), jmax = self._states(x0, xf), f64(jmax).reshape(7); B = x0.shape[0]
        wx, wu, wT = np.zeros((B, self.N, self.nx)), np.zeros((B, self.N, self.nu)), np.zeros(B)
        a0, aT = self._acc(acc0, B), self._acc(accT, B)
        check(lib().mpcmp_warm_start_jerk_lim_batch(self._ctx, B, host(x0), host(xf), host(a0), host(aT), host(self._lim(vmax)),
                                                    host(self._lim(amax)), host(jmax), host(wx), host(wu), host(wT)), self._ctx)
        return wx, wu, wT

    def warm_start_jerk_device(self, B, x0, xf, jmax, warm_x, warm_u, warm_T, stream=0):
        """Device-pointer form: writes the warm start where solve_device(..., warm=(warm_x, warm_u, warm_T)) reads it."""
        jmax = f64(jmax)
        check(lib().mpcmp_warm_start_jerk_batch_device(self._ctx, int(B), x0 or None, xf or None, host(jmax), warm_x or None, warm_u or None,
                                                       warm_T or None, stream or None), self._ctx)

    def jerk_trajectory(self, x0, xf, jmax, n_pts=200, acc0=None, accT=None, vmax=None, amax=None):
        """The same trajectory sampled uniformly: out [B][n_pts+1][22] = t, q, qd, qdd, and the durations [B]."""
        (x0, xf), jmax = self._states(x0, xf), f64(jmax).reshape(7); B = x0.shape[0]
        out, T = np.zeros((B, n_pts + 1, 22)), np.zeros(B)
        a0, aT = self._acc(acc0, B), self._acc(accT, B)
        check(lib().mpcmp_jerk_trajectory_lim_batch(self._ctx, B, host(x0), host(xf), host(a0), host(aT), host(self._lim(vmax)),
                                                    host(self._lim(amax)), host(jmax), int(n_pts), host(out), host(T)), self._ctx)
        return out, T

    def jerk_point(self, x0, xf, jmax, time, acc0=None, accT=None, vmax=None, amax=None):
        """MotionPlanner::get_RK_point: [B][28] = q, qd, qdd, tau of the jerk-limited trajectory at min(time, duration), durations [B]."""
        (x0, xf), jmax = self._states(x0, xf), f64(jmax).reshape(7); B = x0.shape[0]
        time = f64(np.broadcast_to(np.asarray(time, dtype=np.float64), (B,)))
        out, T = np.zeros((B, 28)), np.zeros(B)
        a0, aT = self._acc(acc0, B), self._acc(accT, B)
        check(lib().mpcmp_jerk_point_lim_batch(self._ctx, B, host(x0), host(xf), host(a0), host(aT), host(self._lim(vmax)), host(self._lim(amax)),
                                               host(jmax), host(time), host(out), host(T)), self._ctx)
        return out, T

    def mpc_point(self, sx, su, sT, time):
        """MotionPlanner::get_MPC_point (with its clamp: time >= T -> normalised time T): [B][28] = q, qd, qdd, tau."""
        sx, su, sT = self._traj(sx, su, sT); B = sT.shape[0]
        time = f64(np.broadcast_to(np.asarray(time, dtype=np.float64), (B,)))
        out = np.zeros((B, 28))
        check(lib().mpcmp_mpc_point_batch(self._ctx, B, host(sx), host(su), host(sT), host(time), host(out)), self._ctx)
        return out

    def rnea(self, q, qd, qdd):
        q, qd, qdd = f64(q), f64(qd), f64(qdd); tau = np.zeros_like(q)
        check(lib().mpcmp_rnea_batch(self._ctx, q.shape[0], host(q), host(qd), host(qdd), host(tau)), self._ctx)
        return tau

    def eval_constraints(self, x, u):
        x, u = f64(x), f64(u); nn = x.shape[0]
        g, G = np.zeros((nn, 8)), np.zeros((nn, 8, 22))
        check(lib().mpcmp_eval_constraints_batch(self._ctx, nn, host(x), host(u), host(g), host(G)), self._ctx)
        return g, G

    def qp(self, x0, xf, xs, us, T):
        x0, xf = self._states(x0, xf); B = x0.shape[0]
        xs, us, T = self._traj(xs, us, T)
        if T.shape[0] != B:
            raise ValueError("linearisation point is for %d problems, states for %d" % (T.shape[0], B))
        p, y = np.zeros((B, self.n)), np.zeros((B, self.m + self.n)); it = np.zeros(B, dtype=np.int32)
        check(lib().mpcmp_qp_batch(self._ctx, B, host(x0), host(xf), host(xs), host(us), host(T), host(p), host(y), host(it)), self._ctx)
        return p, y, it

    def sample(self, sx, su, sT, n_pts=200):
        sx, su, sT = self._traj(sx, su, sT); B = sx.shape[0]
        out = np.zeros((B, n_pts + 1, 29))
        check(lib().mpcmp_sample_batch(self._ctx, B, host(sx), host(su), host(sT), int(n_pts), host(out)), self._ctx)
        return out

    def sample_device(self, B, sol_x, sol_u, sol_T, n_pts, out, stream=0):
        check(lib().mpcmp_sample_batch_device(self._ctx, int(B), sol_x or None, sol_u or None, sol_T or None, int(n_pts), out or None,
                                              stream or None), self._ctx)

    def traj_stats(self, sx, su, sT, xf, n_pts=200):
        (sx, su, sT), xf = self._traj(sx, su, sT), f64(xf); B = sx.shape[0]
        if xf.shape != (B, 14):
            raise ValueError("xf must be [B][14]")
        out = np.zeros((B, 74))
        check(lib().mpcmp_traj_stats_batch(self._ctx, B, host(sx), host(su), host(sT), host(xf), int(n_pts), host(out)), self._ctx)
        return out

    def reset_multipliers(self):
        """zero the multipliers every problem slot carries to its next solve (mpcmp_config.carry_multipliers)"""
        check(lib().mpcmp_reset_multipliers(self._ctx), self._ctx)

    # -- receding horizon (BASELINE config #5)
    def rh_init(self, x0, xf):
        x0, xf = self._states(x0, xf)
        self._rh_B = x0.shape[0]
        check(lib().mpcmp_rh_init(self._ctx, self._rh_B, host(x0), host(xf)), self._ctx)

    def rh_run(self, steps, dt, use_graph=True):
        check(lib().mpcmp_rh_run(self._ctx, int(steps), float(dt), int(bool(use_graph))), self._ctx)

    def rh_get(self):
        B = self._rh_B
        x0 = np.zeros((B, self.nx)); sx, su, sT = np.zeros((B, self.N, self.nx)), np.zeros((B, self.N, self.nu)), np.zeros(B)
        info = np.zeros(B, dtype=capi.INFO_DTYPE)
        check(lib().mpcmp_rh_get(self._ctx, host(x0), host(sx), host(su), host(sT), host(info)), self._ctx)
        return x0, sx, su, sT, info

    def rh_stats(self):
        """(re-solves executed on live instances, instances retired) since rh_init (mpcmp_rh_stats)"""
        done, arr = C.c_longlong(0), C.c_longlong(0)
        check(lib().mpcmp_rh_stats(self._ctx, C.byref(done), C.byref(arr)), self._ctx)
        return int(done.value), int(arr.value)

    def rh_update(self, idx=None, x=None, xf=None, restart=False):
        """between two rh_run calls: new measured states x [n][nx] and / or targets xf [n][nx] of the instances idx [n] (None: all B, in order);
        a new target, restart=True or a retired instance restarts from the driver's start guess (mpcmp_rh_update, include/mpcmp.h)"""
        x, xf = [None if v is None else f64(v).reshape(-1, self.nx) for v in (x, xf)]
        if idx is not None:
            idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))
        rows = [v.shape[0] for v in (idx, x, xf) if v is not None]
        if len(set(rows)) > 1:
            raise ValueError("idx, x and xf must list the same number of instances, got %s" % rows)
        n = rows[0] if rows else getattr(self, "_rh_B", 0)
        check(lib().mpcmp_rh_update(self._ctx, int(n), host(idx), host(x), host(xf), capi.RH_RESTART if restart else 0), self._ctx)

    def rh_update_device(self, n, idx, x, xf, restart=False, stream=0):
        """rh_update with raw device pointers (idx: int32 [n], x / xf: double [n][nx]; 0 = NULL), ordered after the work on `stream`
        (mpcmp_rh_update_device: indices and values are not checked)"""
        check(lib().mpcmp_rh_update_device(self._ctx, int(n), idx or None, x or None, xf or None, capi.RH_RESTART if restart else 0,
                                           stream or None), self._ctx)

    def pose_targets(self, R, p, seeds, q_ref=None, twist=None, arm=0, xf=None):
        """Joint-space targets from tool poses: multi-start DLS inverse kinematics on the GPU (mpcmp_pose_targets_batch, include/mpcmp.h).
        R [B][3][3], p [B][3] desired tool poses; seeds [B][S][7] starts (scenarios.ik_seeds); q_ref [B][7] prefers the qualifying start
        closest to it; twist [B][6] tool velocity [linear; angular] (None: qd = 0).  Writes arm `arm`'s q and qd columns of xf [B][nx]
        (None: a new zero array; else a C-contiguous float64 array, filled in place).  Returns (xf, info) with info of IK_INFO_DTYPE."""
        seeds = f64(seeds)
        if seeds.ndim == 2:
            seeds = seeds[:, None, :]
        B, S = seeds.shape[0], seeds.shape[1]
        if seeds.shape[2] != 7:
            raise ValueError("seeds must be [B][S][7], got %s" % (seeds.shape,))
        R, p = f64(R).reshape(B, 9), f64(p).reshape(B, 3)
        q_ref = None if q_ref is None else f64(q_ref).reshape(B, 7)
        twist = None if twist is None else f64(twist).reshape(B, 6)
        if xf is None:
            xf = np.zeros((B, self.nx))
        elif not (isinstance(xf, np.ndarray) and xf.dtype == np.float64 and xf.flags.c_contiguous and xf.shape == (B, self.nx)):
            raise ValueError("xf must be a C-contiguous float64 array of shape (%d, %d)" % (B, self.nx))
        info = np.zeros(B, dtype=capi.IK_INFO_DTYPE)
        check(lib().mpcmp_pose_targets_batch(self._ctx, int(B), int(arm), host(R), host(p), host(twist), int(S), host(seeds), host(q_ref), host(xf),
                                             host(info)), self._ctx)
        return xf, info

    def pose_targets_device(self, B, arm, R, p, twist, S, seeds, q_ref, xf, info, stream=0):
        """pose_targets with raw device pointers (0 = NULL for twist, q_ref and info), ordered on `stream`; values are not checked
        (mpcmp_pose_targets_batch_device)"""
        check(lib().mpcmp_pose_targets_batch_device(self._ctx, int(B), int(arm), R or None, p or None, twist or None, int(S), seeds or None,
                                                    q_ref or None, xf or None, info or None, stream or None), self._ctx)

    def debug_fetch(self, which, count):
        """diagnostics: first `count` doubles of a workspace array (0 z, 1 lambda, 2 c_eq, 3 g, 4 p, 5 y), device layout"""
        out = np.zeros(int(count))
        check(lib().mpcmp_debug_fetch(self._ctx, int(which), host(out), int(count)), self._ctx)
        return out

    def kernel_timing(self, reset=False):
        name = C.c_char_p(); ms = C.c_double(); nl = C.c_int()
        check(lib().mpcmp_kernel_timing(self._ctx, int(reset), C.byref(name), C.byref(ms), C.byref(nl)), self._ctx)
        return name.value.decode(), ms.value, nl.value


class BatchMotionPlanner:
    """Batched `MotionPlanner`: same member names / argument meaning, arrays carry a leading batch axis.

    Reference call sequence (examples/benchmark.cpp:6-53): MotionPlanner(urdf); set_constraint_margins(...);
    per problem set_current_state / set_target_state; solve_trajectory(true); get_MPC_trajectory<200>.
    """

    eps = 1e-2  # motionPlanner.hpp:44

    def __init__(self, urdf_path=None, max_batch=1024, num_seg=4, sqp_iters=20, device=0):
        self.model = capi.model_from_urdf(urdf_path) if urdf_path else capi.default_model()
        self.limits = capi.default_limits()
        self.cfg = capi.default_config(num_seg, sqp_iters)         # motionPlanner.cpp:15-24
        self._solver = Solver(self.cfg, max_batch, device, self.model)
        mid = 0.5 * (self.limits["qmin"] + self.limits["qmax"])    # motionPlanner.cpp:5-8
        self.current_state = np.concatenate([mid, np.zeros(7)])[None, :]
        self.target_state = self.current_state.copy()
        self.margin_position_ = self.margin_velocity_ = self.margin_acceleration_ = 1.0
        self.margin_torque_ = self.margin_jerk_ = 1.0
        self._warm = None
        self._sol = None
        self._rk = None
        self._payload = None
        self._via = None
        self._route = None
        self._line = None                       # the goal poses of the last plan_tool_line, while its plans are the last solution

    # motionPlanner.cpp:56-90
    def set_constraint_margins(self, margin_position, margin_velocity, margin_acceleration, margin_torque, margin_jerk):
        self.margin_position_, self.margin_velocity_ = margin_position, margin_velocity
        self.margin_acceleration_, self.margin_torque_, self.margin_jerk_ = margin_acceleration, margin_torque, margin_jerk
        check(lib().mpcmp_set_margins(C.byref(self.cfg), float(margin_position), float(margin_velocity), float(margin_acceleration),
                                      float(margin_torque)))
        self._solver.set_config(self.cfg)

    # motionPlanner.cpp:92-100
    def set_min_height(self, min_height):
        check(lib().mpcmp_set_min_height(C.byref(self.cfg), float(min_height)))
        self._solver.set_config(self.cfg)

    # motionPlanner.cpp:27-39 / 41-54
    def set_target_state(self, target_position, target_velocity):
        self.target_state = np.concatenate([f64(target_position), f64(target_velocity)], axis=-1).reshape(-1, 14)

    def set_current_state(self, current_position, current_velocity):
        self.current_state = np.concatenate([f64(current_position), f64(current_velocity)], axis=-1).reshape(-1, 14)

    # motionPlanner.cpp:116-144
    def check_state_in_bounds(self, position, velocity, acceleration=None):
        position, velocity = f64(position), f64(velocity)
        L = self.limits
        s = (1 - self.margin_position_) * (L["qmax"] - L["qmin"]) / 2
        pc = np.any(position > L["qmax"] - s, axis=-1) | np.any(position < L["qmin"] + s, axis=-1)
        vc = np.any(np.abs(velocity) > self.margin_velocity_ * L["vmax"], axis=-1)
        flag = np.where(pc & ~vc, 1, 0) + np.where(~pc & vc, 2, 0) + np.where(pc & vc, 3, 0)
        if acceleration is not None:
            flag = flag + 10 * np.any(np.abs(f64(acceleration)) > self.margin_acceleration_ * L["amax"], axis=-1)
        return flag

    # motionPlanner.hpp:145-172 (generic warm start from a regularly time-spaced trajectory [B, nPoint, 7])
    def warm_start(self, final_time, position_trajectory, velocity_trajectory, acceleration_trajectory):
        q, v, a = f64(position_trajectory), f64(velocity_trajectory), f64(acceleration_trajectory)
        nP = q.shape[1]
        idx = np.floor(capi.time_nodes(self.cfg.num_seg) * (nP - 1) + 0.5).astype(int)     # std::round, motionPlanner.hpp:157
        self._warm = (np.concatenate([q[:, idx], v[:, idx]], axis=-1), a[:, idx], f64(final_time).reshape(-1))

    # extension beyond the reference's members: the load the gripper carries (include/mpcmp.h, mpcmp_set_payloads)
    def set_payload(self, mass, com=None, inertia=None):
        """payload for the next solve_trajectory and the MPC samples of its solution: mass scalar or [B], com [3] or [B,3] (joint-7 frame,
        default the tool point), inertia about the COM [3,3] or [B,3,3] (default 0); mass None removes it.  Scalars apply to every problem."""
        if mass is None:
            self._payload = None
            self._solver.clear_payloads()
            return
        m = f64(mass).reshape(-1)
        c = None if com is None else f64(com).reshape(-1, 3)
        I = None if inertia is None else f64(inertia).reshape(-1, 3, 3)
        self._payload = (m, c, I)

    def _apply_payload(self, B):
        if self._payload is None:
            return
        m, c, I = self._payload
        self._solver.set_payloads(np.broadcast_to(m, (B,)), None if c is None else np.broadcast_to(c, (B, 3)),
                                  None if I is None else np.broadcast_to(I, (B, 3, 3)))

    # extension beyond the reference's members: a final-time window per problem (include/mpcmp.h, mpcmp_set_time_windows)
    def set_final_time_window(self, lbT, ubT=None):
        """window of the final time for the next solve_trajectory: scalars or [B] (lbT == ubT: exactly that duration); lbT None removes it"""
        if lbT is None:
            self._twin = None
            self._solver.clear_time_windows()
            return
        self._twin = (f64(lbT).reshape(-1), f64(lbT if ubT is None else ubT).reshape(-1))

    # extension beyond the reference's members: the world the plans run in (include/mpcmp.h, clearance)
    def set_obstacles(self, obstacles, sphere_radius=0.06, sphere_spacing=0.08, spheres=None):
        """obstacles: capi.OBSTACLE_DTYPE [n_obs] or [B][n_obs]; None removes them.  The robot is `spheres` (capi.SPHERE_DTYPE) or, by default,
        the skeleton of capi.link_spheres(model, sphere_radius, sphere_spacing)"""
        if obstacles is None:
            self._solver.clear_obstacles()
            self._has_obstacles = False
            return
        self._spheres = capi.link_spheres(self.model, sphere_radius, sphere_spacing) if spheres is None else spheres
        self._solver.set_robot_spheres(self._spheres)
        self._solver.set_obstacles(obstacles)
        self._has_obstacles = True

    def check_clearance(self, n_pts=200, margin=0.0, self_gap=0):
        """clearance records (capi.CLEARANCE_DTYPE [B]) of the last solve_trajectory's solutions; of routes: the legs' records joined per route"""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            clr = self._solver.clearance(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_T"].reshape(L), n_pts, margin, self_gap)
            return self._solver.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr.reshape(r["sol_T"].shape))[3]
        return self._solver.clearance(self._sol[0], self._sol[2], n_pts, margin, self_gap)

    # -- voxel worlds (include/mpcmp_field.h): what a depth camera saw as the world, beside or instead of the primitives of set_obstacles
    def _field_spheres(self, sphere_radius, sphere_spacing, spheres):
        if spheres is not None or getattr(self, "_spheres", None) is None:
            self._spheres = capi.link_spheres(self.model, sphere_radius, sphere_spacing) if spheres is None else spheres
            self._solver.set_robot_spheres(self._spheres)

    def set_voxel_world(self, origin, h, occ, sphere_radius=0.06, sphere_spacing=0.08, spheres=None):
        """an occupancy grid occ [n2][n1][n0] (nonzero: solid) of cubes of edge h whose lowest corner is `origin`; occ None removes the voxel world.
        The robot is the sphere table already in force, `spheres`, or the skeleton of capi.link_spheres(model, sphere_radius, sphere_spacing)"""
        if occ is None:
            self._solver.set_field(None)
            return
        occ = np.asarray(occ)
        if occ.ndim != 3:
            raise ValueError("occ must be [n2][n1][n0], got %s" % (occ.shape,))
        self._field_spheres(sphere_radius, sphere_spacing, spheres)
        self._solver.set_field(capi.field_desc(origin, h, occ.shape[::-1]), occ)

    def set_point_cloud(self, origin, h, n, points, sphere_radius=0.06, sphere_spacing=0.08, spheres=None):
        """a point cloud points [n_points][3] (world frame) as the world: the voxels of the grid (origin, h, n = (n0, n1, n2)) that contain a
        point are solid; points outside the grid and non-finite points are skipped"""
        self._field_spheres(sphere_radius, sphere_spacing, spheres)
        self._solver.set_field_points(capi.field_desc(origin, h, n), points)

    # -- camera frames (include/mpcmp_frame.h): the same worlds with the robot itself, seen by the camera at the posture robot_q, removed.
    # robot_pad above 4.34 h + margin (clouds, images) or 3.47 h + margin (grids) makes that posture clear of the frame by construction
    frame_stats = None      # the counts of the last of the three calls below, a dict

    def set_point_cloud_filtered(self, origin, h, n, points, robot_q, robot_pad, keep=False, sphere_radius=0.06, sphere_spacing=0.08, spheres=None):
        """set_point_cloud without the points within r_s + robot_pad of a robot sphere at robot_q [7] (None: no filter); keep: the cloud is added
        to the world in force (a second camera, or a camera on top of set_voxel_world).  The counts are kept in frame_stats and returned"""
        self._field_spheres(sphere_radius, sphere_spacing, spheres)
        self.frame_stats = self._solver.set_field_points_filtered(capi.field_desc(origin, h, n), points, robot_q, robot_pad, keep)
        return self.frame_stats

    def set_depth_image(self, origin, h, n, camera, depth, robot_q=None, robot_pad=0.0, keep=False, sphere_radius=0.06, sphere_spacing=0.08,
                        spheres=None):
        """a depth image depth [height][width] (uint16 or float) of capi.camera(...) as the world: unprojected, filtered and marked on the GPU"""
        self._field_spheres(sphere_radius, sphere_spacing, spheres)
        self.frame_stats = self._solver.set_field_depth(capi.field_desc(origin, h, n), camera, depth, robot_q, robot_pad, keep)
        return self.frame_stats

    def carve_robot(self, robot_q, robot_pad, sphere_radius=0.06, sphere_spacing=0.08, spheres=None):
        """the robot at robot_q removed from the voxel world in force (set_voxel_world, a map): occupied voxels whose centre lies within
        r_s + robot_pad of a sphere are cleared"""
        self._field_spheres(sphere_radius, sphere_spacing, spheres)
        self.frame_stats = self._solver.field_carve(robot_q, robot_pad)
        return self.frame_stats

    def check_clearance_field(self, n_pts=200, margin=0.0, merge=True, self_gap=0):
        """clearance records (capi.CLEARANCE_DTYPE [B]) of the last solve_trajectory's solutions against the voxel world; of routes: the legs'
        records joined per route.  merge: when obstacles are set (set_obstacles) or self_gap > 0, the records are merged with those of
        check_clearance(n_pts, margin, self_gap), and (records, source [B]) is returned: source 1 where d_min is the field's and `other` a voxel"""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            clr = self._solver.clearance_field(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_T"].reshape(L), n_pts, margin)
            fld = self._solver.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr.reshape(r["sol_T"].shape))[3]
        else:
            fld = self._solver.clearance_field(self._sol[0], self._sol[2], n_pts, margin)
        if not merge or not (getattr(self, "_has_obstacles", False) or self_gap > 0):
            return fld
        return self._solver.clearance_merge(self.check_clearance(n_pts, margin, self_gap), fld)

    # -- clearance in a moving world (include/mpcmp_moving.h): direct moves; a route's leg slots are checked with Solver.clearance_timed, each with
    # t_start = the route's start plus the running times of the legs before it
    def set_moving_obstacles(self, track_of, offsets, t0, dt):
        """which of the obstacles of set_obstacles move, and how: track_of [n_obs] or [B][n_obs] (-1: stands still), offsets [n_tracks][n_key][3]
        or [B][n_tracks][n_key][3] on the world clock t0 + k dt.  None: the world stands still again (as after the next set_obstacles)"""
        self._solver.set_obstacle_tracks(track_of, offsets, t0, dt)

    def _timed_plans(self, retimed, who):
        if self._route is not None or self._sol is None:
            raise ValueError("%s: direct moves only, after solve_trajectory (check a route's leg slots with Solver.clearance_timed)" % who)
        if retimed and getattr(self, "_retimed", None) is None:
            raise ValueError("%s: call retime() first" % who)
        return self._sol[0], self._sol[2], (self._retimed[0] if retimed else None)

    def check_clearance_timed(self, t_start=None, n_pts=200, margin=0.0, self_gap=0, retimed=False):
        """clearance records (capi.CLEARANCE_DTYPE [B]) of the last solve_trajectory's solutions started at the world times t_start (a scalar, [B] or
        None: 0) in the moving world; retimed: run on the profiles of the last retime().  Times are on the running clock"""
        sx, sT, prof = self._timed_plans(retimed, "check_clearance_timed")
        return self._solver.clearance_timed(sx, sT, prof, t_start, n_pts, margin, self_gap)

    def first_clear_start(self, delays, check_wait=True, n_pts=200, margin=0.0, self_gap=0, retimed=False):
        """(capi.START_DELAY_DTYPE [B], d_min_all [B][K]): per plan the lowest of the candidate start delays [K] whose run is clear of the moving
        world; check_wait: the wait at the start posture is checked at the candidate delays too"""
        sx, sT, prof = self._timed_plans(retimed, "first_clear_start")
        return self._solver.start_delay(sx, sT, delays, prof, check_wait, n_pts, margin, self_gap)

    def check_clearance_certified_timed(self, t_start=None, wait_before=None, hold_after=None, margin=0.0, self_gap=0, n_start=4, n_rest=4,
                                        max_depth=10, retimed=False):
        """certified clearance of the last solve_trajectory's solutions in the moving world (include/mpcmp_moving_cert.h): (capi.CLEARANCE_DTYPE [B],
        capi.CLEARANCE_CERT_DTYPE [B]).  The motion starts at the world time t_start after a wait of wait_before at the start posture and is followed
        by a hold of hold_after at the target (each a scalar, [B] or None: 0); status 0 holds at every world time of that span, not at samples.
        Direct moves on their own clock only: the certificate does not survive retiming"""
        if retimed:
            raise ValueError("check_clearance_certified_timed: there is no certificate on a retimed clock (the rule has no retime profile); check the "
                             "plan on its own clock, or sample the retimed plan with check_clearance_timed(retimed=True)")
        if self._route is not None or self._sol is None:
            raise ValueError("check_clearance_certified_timed: direct moves only, after solve_trajectory (check a route's leg slots with "
                             "Solver.clearance_certified_timed, each with t_start = the route's start plus the durations of the legs before it)")
        return self._solver.clearance_certified_timed(self._sol[0], self._sol[2], t_start, wait_before, hold_after, margin, self_gap, n_start, n_rest,
                                                      max_depth)

    def first_certified_start(self, delays, margin=0.0, self_gap=0, n_pts=200, hold_after=None, n_start=4, n_rest=4, max_depth=10, max_rounds=4):
        """(index [B], capi.CLEARANCE_DTYPE [B], capi.CLEARANCE_CERT_DTYPE [B]): per plan the lowest of the candidate start delays [K] that
        first_clear_start(check_wait=True) calls clear AND whose certified record (t_start = delays[k], wait_before = delays[k] - delays[0]) has status
        0; -1: none within max_rounds candidates.  A host loop over the two checks: a problem whose record is not 0 moves to its next sampled-clear
        candidate.  The records are those of the last candidate tried (all zero for a problem without any sampled-clear delay)"""
        delays = np.asarray(delays, dtype=np.float64).reshape(-1)
        _, d_all = self.first_clear_start(delays, True, n_pts, margin, self_gap)
        B = d_all.shape[0]
        cand = [list(np.nonzero(~(d_all[b] < margin))[0]) for b in range(B)]
        pos, index = np.zeros(B, dtype=int), np.full(B, -1, dtype=int)
        pending = np.array([len(c) > 0 for c in cand])
        clr, cert = np.zeros(B, dtype=capi.CLEARANCE_DTYPE), np.zeros(B, dtype=capi.CLEARANCE_CERT_DTYPE)
        for _ in range(int(max_rounds)):
            if not pending.any():
                break
            k = np.array([cand[b][pos[b]] if pending[b] else 0 for b in range(B)])
            c, ce = self.check_clearance_certified_timed(delays[k], delays[k] - delays[0], hold_after, margin, self_gap, n_start, n_rest, max_depth)
            clr[pending], cert[pending] = c[pending], ce[pending]
            ok = pending & (c["status"] == 0)
            index[ok] = k[ok]
            pending &= ~ok
            pos[pending] += 1
            pending &= np.array([pos[b] < len(cand[b]) for b in range(B)])
        return index, clr, cert

    def plan_as_moving_world(self, other, obstacles=None, t_start=None, n_key=256, horizon=None, retimed=False):
        """This planner's last plans become the moving world of the planner `other` (prioritised planning: `other` is checked against them): problem
        b of `other` sees the obstacles `obstacles` (capi.OBSTACLE_DTYPE [n_obs], standing still; None: none) and this robot's spheres, moving as
        plan b does when started at the world time t_start (a scalar, [B] or None: 0), held at its first / last posture outside the plan.  The
        tracks have n_key keys from world time 0 to `horizon` (default: the latest end of a plan).  Returns the tracks [B][nsph][n_key][3]"""
        sx, sT, prof = self._timed_plans(retimed, "plan_as_moving_world")
        B = sT.shape[0]
        if getattr(self, "_spheres", None) is None:
            self._spheres = capi.link_spheres(self.model, 0.06, 0.08)
            self._solver.set_robot_spheres(self._spheres)
        ts = np.zeros(B) if t_start is None else np.broadcast_to(np.asarray(t_start, dtype=np.float64), (B,))
        T_run = prof[:, -1, 0] if retimed else sT
        if horizon is None:
            horizon = float(np.max(ts + T_run))
        dt = horizon / max(int(n_key) - 1, 1) if horizon > 0 else 1.0
        tracks = self._solver.sphere_tracks(sx, sT, 0.0, dt, n_key, prof, ts)
        still = np.zeros(0, dtype=capi.OBSTACLE_DTYPE) if obstacles is None else capi._records(obstacles, capi.OBSTACLE_DTYPE, "obstacle").reshape(-1)
        mine = np.array([capi.obstacle(capi.OBS_SPHERE, (0, 0, 0), (0, 0, 0), float(r)) for r in self._spheres["r"]], dtype=capi.OBSTACLE_DTYPE)
        world = np.ascontiguousarray(np.broadcast_to(np.concatenate([still, mine]), (B, still.shape[0] + mine.shape[0])))
        track_of = np.concatenate([np.full(still.shape[0], -1), np.arange(mine.shape[0])]).astype(np.int32)
        other.set_obstacles(world) if getattr(other, "_spheres", None) is None else other.set_obstacles(world, spheres=other._spheres)
        other.set_moving_obstacles(np.broadcast_to(track_of, (B, track_of.shape[0])), tracks, 0.0, dt)
        return tracks

    def check_clearance_certified(self, margin=0.0, self_gap=0, n_start=4, max_depth=10):
        """certified clearance of the last solve_trajectory's solutions: (capi.CLEARANCE_DTYPE [B], capi.CLEARANCE_CERT_DTYPE); status 0 holds at every
        time of the plan, not at samples.  Of routes: the legs' records joined per route [B] (an undecided or hit leg marks its route) and the
        certificates per leg [B][M + 1] (times are leg times)"""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            clr, cert = self._solver.clearance_certified(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_T"].reshape(L), margin, self_gap, n_start,
                                                         max_depth)
            return self._solver.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr.reshape(r["sol_T"].shape))[3], cert.reshape(r["sol_T"].shape)
        return self._solver.clearance_certified(self._sol[0], self._sol[2], margin, self_gap, n_start, max_depth)

    def check_clearance_certified_field(self, margin=0.0, n_start=4, max_depth=10, merge=True, self_gap=0):
        """certified clearance of the last solve_trajectory's solutions against the voxel world (include/mpcmp_field_cert.h): (capi.CLEARANCE_DTYPE
        [B], capi.CLEARANCE_CERT_DTYPE); status 0 holds at every time of the plan.  Of routes: the legs' records joined per route [B] and the
        certificates per leg [B][M + 1], as check_clearance_certified.  merge: when obstacles are set (set_obstacles) or self_gap > 0, both records
        are merged with those of check_clearance_certified(margin, self_gap, n_start, max_depth), and (records, certificates, source [B]) is returned:
        source 1 where d_min is the field's and `other` a voxel"""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            clr, cert = self._solver.clearance_certified_field(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_T"].reshape(L), margin, n_start,
                                                               max_depth)
            clr = self._solver.route_join(r["sol_x"], r["sol_u"], r["sol_T"], r["info"], clr.reshape(r["sol_T"].shape))[3]
            cert = cert.reshape(r["sol_T"].shape)
        else:
            clr, cert = self._solver.clearance_certified_field(self._sol[0], self._sol[2], margin, n_start, max_depth)
        if not merge or not (getattr(self, "_has_obstacles", False) or self_gap > 0):
            return clr, cert
        pclr, pcert = self.check_clearance_certified(margin, self_gap, n_start, max_depth)
        mclr, src = self._solver.clearance_merge(pclr, clr)
        mcert = self._solver.clearance_cert_merge(np.ascontiguousarray(pcert).reshape(-1), np.ascontiguousarray(cert).reshape(-1)).reshape(cert.shape)
        return mclr, mcert, src

    def check_limits(self, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """limit records (capi.LIMITS_DTYPE) of the last solve_trajectory's solutions between their nodes, [B]; of routes: one record per leg,
        [B][M + 1] (times are leg times)"""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            lim = self._solver.limits(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_u"].reshape(L, self._solver.N, 7), r["sol_T"].reshape(L),
                                      n_pts, tol, tool_lin_max, tool_ang_max)
            return lim.reshape(r["sol_T"].shape)
        return self._solver.limits(self._sol[0], self._sol[1], self._sol[2], n_pts, tol, tool_lin_max, tool_ang_max)

    def retime(self, n_grid=200, spec=None):
        """the last solve_trajectory's solutions retimed along their own paths (Solver.retime): (prof [B][n_grid + 1][2], capi.RETIME_DTYPE [B]); of
        routes: leg by leg, ([B][M + 1][n_grid + 1][2], [B][M + 1]) with leg times.  The profiles are kept for get_retimed_trajectory."""
        if self._route is not None:
            r = self._route
            L = r["sol_T"].size
            prof, rec = self._solver.retime(r["sol_x"].reshape(L, self._solver.N, 14), r["sol_u"].reshape(L, self._solver.N, 7),
                                            r["sol_T"].reshape(L), n_grid, spec)
            return prof.reshape(r["sol_T"].shape + prof.shape[1:]), rec.reshape(r["sol_T"].shape)
        self._retimed = self._solver.retime(self._sol[0], self._sol[1], self._sol[2], n_grid, spec)
        return self._retimed

    def get_retimed_trajectory(self, n_pts=200):
        """get_MPC_trajectory on the retimed clock: [B][n_pts + 1][1 + 28 narm] from the profiles of the last retime call (direct moves)"""
        if self._route is not None or getattr(self, "_retimed", None) is None:
            raise ValueError("call retime() after solve_trajectory() first (direct moves)")
        return self._solver.sample_retimed(self._sol[0], self._sol[1], self._sol[2], self._retimed[0], n_pts)

    def check_retimed_limits(self, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """limit records of the retimed plans between the grid points (Solver.limits_retimed), from the profiles of the last retime call (direct
        moves): (capi.LIMITS_DTYPE [B], T_new [B])"""
        if self._route is not None or getattr(self, "_retimed", None) is None:
            raise ValueError("call retime() after solve_trajectory() first (direct moves)")
        return self._solver.limits_retimed(self._sol[0], self._sol[1], self._sol[2], self._retimed[0], n_pts, tol, tool_lin_max, tool_ang_max)

    def retime_route(self, n_grid=200, spec=None):
        """the last route solve retimed as whole routes, one profile across the via points (Solver.retime_route): (prof [B][M + 1][n_grid + 1][2]
        with leg times, leg_T_new [B][M + 1], capi.ROUTE_RETIME_DTYPE [B]).  The profiles are kept for get_retimed_route_trajectory."""
        if self._route is None:
            raise ValueError("call set_via_points() and solve_trajectory() first (routes); retime() retimes direct moves")
        r = self._route
        self._route_retimed = (r, self._solver.retime_route(r["sol_x"], r["sol_u"], r["sol_T"], n_grid, spec))
        return self._route_retimed[1]

    def get_retimed_route_trajectory(self, n_pts=200):
        """get_MPC_trajectory on the retimed clock of the route: [B][n_pts + 1][29] from the profiles of the last retime_route call"""
        kept = getattr(self, "_route_retimed", None)
        if self._route is None or kept is None or kept[0] is not self._route:       # (a profile belongs to the route it was computed for)
            raise ValueError("call retime_route() after a route solve first")
        r = self._route
        return self._solver.sample_retimed_route(r["sol_x"], r["sol_u"], r["sol_T"], kept[1][0], n_pts)

    def check_retimed_route_limits(self, n_pts=200, tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
        """limit records of the retimed routes between the grid points (Solver.limits_retimed_route), from the profiles of the last retime_route call:
        (capi.LIMITS_DTYPE [B], T_new [B]), times on the route clock"""
        kept = getattr(self, "_route_retimed", None)
        if self._route is None or kept is None or kept[0] is not self._route:       # (a profile belongs to the route it was computed for)
            raise ValueError("call retime_route() after a route solve first")
        r = self._route
        return self._solver.limits_retimed_route(r["sol_x"], r["sol_u"], r["sol_T"], kept[1][0], n_pts, tol, tool_lin_max, tool_ang_max)

    # extension beyond the reference's members: a straight tool line as the plan (include/mpcmp_toolpath.h)
    def plan_tool_line(self, R, p, T=None, spec=None):
        """straight tool lines from the current states' postures to the poses R [B][3][3], p [B][3] (Solver.tool_line), stored as the last solution:
        check_limits, check_clearance, retime, get_retimed_trajectory and get_MPC_trajectory then apply to them.  Returns capi.TOOL_LINE_DTYPE [B]."""
        R = f64(R).reshape(-1, 3, 3); B = max(R.shape[0], self.current_state.shape[0])
        q = np.ascontiguousarray(np.broadcast_to(self.current_state[:, :7], (B, 7)))
        sx, su, sT, rec = self._solver.tool_line(q, np.broadcast_to(R, (B, 3, 3)), np.broadcast_to(f64(p).reshape(-1, 3), (B, 3)), T, spec)
        self._route = None
        self._sol = (sx, su, sT)
        self._retimed = None
        self._warm = (sx.copy(), su.copy(), sT.copy())      # (a tool line is a legal start guess of the next solve)
        self._line = (np.array(np.broadcast_to(R, (B, 3, 3))), np.array(np.broadcast_to(f64(p).reshape(-1, 3), (B, 3))))
        return rec

    def check_tool_line(self, n_pts=200, tol_lin=np.inf, tol_ang=np.inf):
        """deviation records (capi.TOOL_DEV_DTYPE [B]) of the last plan_tool_line's plans from their lines"""
        if self._route is not None or self._line is None or self._sol is None:
            raise ValueError("call plan_tool_line() first")
        return self._solver.tool_deviation(self._sol[0], self._line[0], self._line[1], n_pts, tol_lin, tol_ang)

    # extension beyond the reference's members: a move through via points (include/mpcmp.h, "via-point routes")
    def set_via_points(self, via, via_velocity=None, speed=0.5):
        """via [B][M][7] (or [M][7] for every problem): the next solve_trajectory plans x0 -> via_0 -> .. -> xf without stopping, and
        get_MPC_trajectory samples the route.  via_velocity [B][M][7]: the joint velocities at the vias; None: the chord rule at `speed` in [0, 1].
        via None: back to direct moves.  Payloads, windows and obstacle sets given per problem apply to every leg of its route; with per-problem
        obstacle SETS, repeat each set M + 1 times (Solver.repeat)."""
        if via is None:
            self._via = self._route = None
            return
        via = f64(via)
        self._via = (via if via.ndim == 3 else via[None], None if via_velocity is None else f64(via_velocity).reshape(-1, via.shape[-2], 7), speed)

    # motionPlanner.cpp:177-208
    def solve_trajectory(self, use_builtin_warm_start=True):
        B = max(self.current_state.shape[0], self.target_state.shape[0])
        self._apply_payload(B)
        if getattr(self, "_twin", None) is not None:
            self._solver.set_time_windows(np.broadcast_to(self._twin[0], (B,)), np.broadcast_to(self._twin[1], (B,)))
        x0 = np.broadcast_to(self.current_state, (B, 14)); xf = np.broadcast_to(self.target_state, (B, 14))
        if self._via is not None:
            return self._solve_route(B, x0, xf, use_builtin_warm_start)
        self._route = None
        if use_builtin_warm_start:      # what the reference gets from Ruckig (warm_start_RK, motionPlanner.cpp:146-175)
            self._rk = (np.array(x0), np.array(xf))
            warm = self._solver.warm_start_jerk(x0, xf, self.margin_jerk_ * self.limits["jmax"])     # motionPlanner.cpp:86-88
        else:
            warm = self._warm
        sx, su, sT, info = self._solver.solve(x0, xf, warm)
        self._sol = (sx, su, sT)
        self._retimed = None                    # (a profile belongs to the plan it was computed for)
        self._line = None
        # re-guess with exact end states (motionPlanner.cpp:199-207)
        gx = sx.copy(); gx[:, 0] = x0; gx[:, -1] = xf
        self._warm = (gx, su.copy(), sT.copy())
        self.info = info
        return info

    def _solve_route(self, B, x0, xf, jerk_start):
        via, vqd, speed = self._via
        M = via.shape[1]; rep = self._solver.repeat
        via = np.broadcast_to(via, (B, M, 7)); vqd = None if vqd is None else np.broadcast_to(vqd, (B, M, 7))
        if self._payload is not None:           # rows are per leg slot: every route's row M + 1 times
            m, c, I = self._payload
            self._solver.set_payloads(rep(np.broadcast_to(m, (B,)), M), None if c is None else rep(np.broadcast_to(c, (B, 3)), M),
                                      None if I is None else rep(np.broadcast_to(I, (B, 3, 3)), M))
        if getattr(self, "_twin", None) is not None:
            self._solver.set_time_windows(rep(np.broadcast_to(self._twin[0], (B,)), M), rep(np.broadcast_to(self._twin[1], (B,)), M))
        r = self._solver.solve_route(x0, via, xf, vqd, speed, self.margin_jerk_ * self.limits["jmax"] if jerk_start else None)
        self._route = r
        self._sol = self._warm = self._line = None      # (the re-guess rule is that of a single move)
        self.info = r["route_info"]
        return self.info

    def solution(self):
        """(sol_x, sol_u, sol_T) of the last solve; of routes: the legs' [B][M+1][..] arrays"""
        if self._route is not None:
            return self._route["sol_x"], self._route["sol_u"], self._route["sol_T"]
        return self._sol

    # motionPlanner.hpp:118-128 / 130-142
    def get_MPC_point(self, time):
        o = self._solver.mpc_point(*self._sol, time=time)
        return o[:, :7], o[:, 7:14], o[:, 14:21], o[:, 21:]

    def get_RK_point(self, time):
        o, _ = self._solver.jerk_point(self._rk[0], self._rk[1], self.margin_jerk_ * self.limits["jmax"], time)
        return o[:, :7], o[:, 7:14], o[:, 14:21], o[:, 21:]

    # motionPlanner.hpp:73-96
    def get_ruckig_trajectory(self, n_pts=200):
        out, _ = self._solver.jerk_trajectory(self._rk[0], self._rk[1], self.margin_jerk_ * self.limits["jmax"], n_pts)
        q, v, a = out[..., 1:8], out[..., 8:15], out[..., 15:22]
        if self._payload is not None:          # (the jerk-limited trajectory is the unloaded comparison: its torques are the model's own)
            self._solver.clear_payloads()
        try:
            tau = self._solver.rnea(q.reshape(-1, 7), v.reshape(-1, 7), a.reshape(-1, 7)).reshape(q.shape)
        finally:
            if self._payload is not None and self._sol is not None:
                self._apply_payload(self._sol[2].shape[0])
        return out[..., 0], q, v, a, tau

    # motionPlanner.hpp:99-116
    def get_MPC_trajectory(self, n_pts=200):
        if self._route is not None:
            out = self._solver.sample_route(self._route["sol_x"], self._route["sol_u"], self._route["sol_T"], n_pts=n_pts)
        else:
            out = self._solver.sample(*self._sol, n_pts=n_pts)
        return out[..., 0], out[..., 1:8], out[..., 8:15], out[..., 15:22], out[..., 22:29]
