"""ctypes declarations for include/mpcmp.h."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libmpcmp.so")


class MpcmpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mpcmp error %d: %s" % (code, msg))
        self.code = code


class Model(C.Structure):
    _fields_ = [("R0", C.c_double * 9 * 7), ("p", C.c_double * 3 * 7), ("mass", C.c_double * 7),
                ("com", C.c_double * 3 * 7), ("I", C.c_double * 9 * 7), ("tool", C.c_double * 3),
                ("link8", C.c_double * 3), ("gravity", C.c_double * 3)]


class Payload(C.Structure):
    """mpcmp_payload: a rigid body on the flange (mass, COM and rotational inertia about the COM, in the joint-7 frame), added to body 7"""
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("I", C.c_double * 9)]


class Config(C.Structure):
    _fields_ = [("num_seg", C.c_int), ("sqp_iters", C.c_int), ("qp_iters", C.c_int), ("ls_iters", C.c_int),
                ("check_every", C.c_int), ("quirk_dtau_dT", C.c_int),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double),
                ("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double), ("rho_eq_scale", C.c_double),
                ("ls_eta", C.c_double), ("ls_tau", C.c_double), ("hess_reg", C.c_double), ("eps_target", C.c_double),
                ("lbx", C.c_double * 14), ("ubx", C.c_double * 14), ("lbu", C.c_double * 7), ("ubu", C.c_double * 7),
                ("lbg", C.c_double * 8), ("ubg", C.c_double * 8), ("lbT", C.c_double), ("ubT", C.c_double),
                ("qp_warm_start", C.c_int), ("carry_multipliers", C.c_int)]


class Info(C.Structure):
    _fields_ = [("T", C.c_double), ("viol_l1", C.c_double), ("defect_inf", C.c_double),
                ("path_viol_inf", C.c_double), ("term_err_inf", C.c_double), ("last_alpha", C.c_double),
                ("qp_iters_total", C.c_int), ("sqp_iters", C.c_int), ("status", C.c_int), ("qp_capped", C.c_int)]


# status bits of mpcmp_info.status (include/mpcmp.h)
STATUS_NAN, STATUS_NOT_PD, STATUS_XCH_DEAD, STATUS_QP_CAPPED, STATUS_OUTSIDE_TOL, STATUS_T_OUT_OF_BOX, STATUS_ARRIVED = 1, 2, 4, 8, 16, 32, 64
STATUS_HARD = STATUS_NAN | STATUS_NOT_PD | STATUS_XCH_DEAD        # the solve itself failed (the other bits grade the returned iterate)
RH_RESTART = 1      # flag of mpcmp_rh_update[_device]: the listed instances restart from the driver's start guess

INFO_DTYPE = np.dtype([("T", "f8"), ("viol_l1", "f8"), ("defect_inf", "f8"), ("path_viol_inf", "f8"),
                       ("term_err_inf", "f8"), ("last_alpha", "f8"), ("qp_iters_total", "i4"),
                       ("sqp_iters", "i4"), ("status", "i4"), ("qp_capped", "i4")])

# record and status bits of mpcmp_pose_targets_batch[_device] (mpcmp_ik_info, include/mpcmp.h)
IK_NOT_CONVERGED, IK_Q_OUT_OF_BOUNDS, IK_QD_OUT_OF_BOUNDS = 1, 2, 4
IK_INFO_DTYPE = np.dtype([("err", "f8"), ("seed", "i4"), ("iters", "i4"), ("status", "i4"), ("pad", "i4")])

# records of the clearance checks (mpcmp_sphere, mpcmp_obstacle, mpcmp_clearance; include/mpcmp.h)
SPHERE_DTYPE = np.dtype([("joint", "i4"), ("pad", "i4"), ("c", "f8", 3), ("r", "f8")])
OBSTACLE_DTYPE = np.dtype([("type", "i4"), ("pad", "i4"), ("a", "f8", 3), ("b", "f8", 3), ("r", "f8")])
CLEARANCE_DTYPE = np.dtype([("d_min", "f8"), ("t_min", "f8"), ("t_first", "f8"), ("sphere", "i4"), ("other", "i4"), ("n_hit", "i4"), ("status", "i4")])
OBS_SPHERE, OBS_CAPSULE, OBS_BOX, OBS_HALFSPACE = 0, 1, 2, 3
CLR_HIT, CLR_NAN = 1, 2
# the certified check (mpcmp_clearance_cert, include/mpcmp_clearance_cert.h): 32 bytes; CLR_UNDECIDED is a status bit of CLEARANCE_DTYPE records
CLR_UNDECIDED = 4
CLEARANCE_CERT_DTYPE = np.dtype([("d_lower", "f8"), ("t_lower", "f8"), ("n_eval", "i4"), ("n_clear", "i4"), ("n_undecided", "i4"), ("depth", "i4")])
CLR_CERT_CAPACITY = 4096
# the start-delay search (mpcmp_start_delay, include/mpcmp_moving.h): 32 bytes; the limits of a track table and of the delays
START_DELAY_DTYPE = np.dtype([("delay", "f8"), ("d_min", "f8"), ("index", "i4"), ("n_clear", "i4"), ("status", "i4"), ("pad", "i4")])
MAX_TRACKS, MAX_TRACK_KEYS, MAX_DELAYS = 64, 1024, 256
MAX_SPHERES, MAX_OBSTACLES = 64, 256
# the grid of a voxel world (mpcmp_field_desc, include/mpcmp_field.h): 48 bytes; the field entry of an empty world and the limits of a grid
FIELD_DESC_DTYPE = np.dtype([("origin", "f8", 3), ("h", "f8"), ("n", "i4", 3), ("pad", "i4")])
FIELD_EMPTY, FIELD_MAX_DIM, FIELD_MAX_VOXELS = 0xFFFFFFFF, 1024, 1 << 24
# camera frames (mpcmp_camera, mpcmp_frame_stats, include/mpcmp_frame.h): 160 and 32 bytes; the depth types, the flag and the largest image
CAMERA_DTYPE = np.dtype([("R", "f8", 9), ("t", "f8", 3), ("fx", "f8"), ("fy", "f8"), ("cx", "f8"), ("cy", "f8"), ("depth_scale", "f8"), ("z_min", "f8"),
                         ("z_max", "f8"), ("width", "i4"), ("height", "i4")])
FRAME_STATS_DTYPE = np.dtype([("n_in", "i4"), ("n_invalid", "i4"), ("n_outside", "i4"), ("n_robot", "i4"), ("n_marked", "i4"), ("n_cleared", "i4"),
                              ("pad", "i4", 2)])
DEPTH_U16, DEPTH_F32, FRAME_KEEP, FRAME_MAX_PIXELS = 0, 1, 1, 1 << 22

# records of the between-node limit checks (mpcmp_limits_spec, mpcmp_limits; include/mpcmp.h): 72 and 168 bytes
LIMITS_SPEC_DTYPE = np.dtype([("tol", "f8", 7), ("tool_lin_max", "f8"), ("tool_ang_max", "f8")])
LIMITS_DTYPE = np.dtype([("excess", "f8", 7), ("t_at", "f8", 7), ("stretch", "f8"), ("t_first", "f8"), ("channel", "i4", 7), ("n_viol", "i4"),
                         ("status", "i4"), ("pad", "i4")])
LIM_GROUPS = 7
LIM_Q, LIM_QD, LIM_QDD, LIM_TAU, LIM_HEIGHT, LIM_TOOL_LIN, LIM_TOOL_ANG = range(7)
LIM_NAN = 128       # status bit of mpcmp_limits: a non-finite sample value (bit g: group g over its tolerance)

# records of retiming (mpcmp_retime_spec, mpcmp_retime; include/mpcmp_retime.h): 32 and 40 bytes
RETIME_SPEC_DTYPE = np.dtype([("tool_lin_max", "f8"), ("tool_ang_max", "f8"), ("rate_max", "f8"), ("groups", "i4"), ("pad", "i4")])
RETIME_DTYPE = np.dtype([("T_new", "f8"), ("rate_min", "f8"), ("s_slowest", "f8"), ("k_fail", "i4"), ("n_slowed", "i4"), ("status", "i4"), ("pad", "i4")])
RT_INFEASIBLE, RT_NAN = 1, 128
# the record of a retimed route (mpcmp_route_retime; include/mpcmp_route_retime.h): 48 bytes
ROUTE_RETIME_DTYPE = np.dtype([("T_new", "f8"), ("rate_min", "f8"), ("s_slowest", "f8"), ("leg_slowest", "i4"), ("leg_fail", "i4"), ("k_fail", "i4"),
                               ("n_slowed", "i4"), ("status", "i4"), ("pad", "i4")])
RT_ALL_GROUPS = (1 << LIM_QD) | (1 << LIM_QDD) | (1 << LIM_TAU) | (1 << LIM_TOOL_LIN) | (1 << LIM_TOOL_ANG)

# records of the tool-line moves (mpcmp_tool_line_spec, mpcmp_tool_line, mpcmp_tool_dev; include/mpcmp_toolpath.h): 56, 40 and 48 bytes
TOOL_LINE_SPEC_DTYPE = np.dtype([("tool_lin_max", "f8"), ("tool_ang_max", "f8"), ("T_min", "f8"), ("damp", "f8"), ("manip_min", "f8"), ("eps", "f8"),
                                 ("n_sub", "i4"), ("pad", "i4")])
TOOL_LINE_DTYPE = np.dtype([("err_max", "f8"), ("manip_min", "f8"), ("s_manip", "f8"), ("q_excess", "f8"), ("k_fail", "i4"), ("status", "i4")])
TOOL_DEV_DTYPE = np.dtype([("lin_max", "f8"), ("s_lin", "f8"), ("perp_max", "f8"), ("ang_max", "f8"), ("s_ang", "f8"), ("n_over", "i4"), ("status", "i4")])
TL_STOPPED, TL_Q_OUT_OF_BOUNDS, TD_OVER, TL_NAN = 1, 2, 1, 128

# one row of mpcmp_set_bounds[_device] (mpcmp_bounds, include/mpcmp.h): the six bound tables of Config, in its order
BOUNDS_DTYPE = np.dtype([("lbx", "f8", 14), ("ubx", "f8", 14), ("lbu", "f8", 7), ("ubu", "f8", 7), ("lbg", "f8", 8), ("ubg", "f8", 8)])

# the seam record of a joined route (mpcmp_route_seam, include/mpcmp.h)
ROUTE_SEAM_DTYPE = np.dtype([("state_jump_inf", "f8"), ("acc_jump_inf", "f8"), ("leg_longest", "i4"), ("leg_first_bad", "i4")])

# The whole C ABI, every function include/mpcmp.h declares in the header's order: name -> the kinds of its arguments, "p" = any pointer (a context,
# a struct, an array, a hipStream_t as void *), "i" = int, "d" = double, "l" = long.  lib() declares exactly this to ctypes, so a 64-bit address
# passed as a plain Python integer arrives whole; the CPU test suite checks the table against the header and the library's exports.
ABI = {
    "mpcmp_reset_multipliers": "p",
    # configuration helpers
    "mpcmp_default_model": "p", "mpcmp_model_add_payload": "ppp", "mpcmp_model_from_urdf": "pp", "mpcmp_models_from_urdf": "pipp",
    "mpcmp_default_limits": "pppppp", "mpcmp_default_config": "pii", "mpcmp_set_margins": "pdddd", "mpcmp_set_min_height": "pd",
    "mpcmp_num_nodes": "i", "mpcmp_time_nodes": "ip", "mpcmp_version": "",
    # context
    "mpcmp_create": "ppiip", "mpcmp_create_multi": "ppiiip", "mpcmp_destroy": "p", "mpcmp_set_config": "pp", "mpcmp_last_error": "p",
    # per-problem payloads
    "mpcmp_set_payloads": "pip", "mpcmp_set_payloads_device": "pipp",
    # the hot path
    "mpcmp_solve_batch": "pi" + "p" * 9, "mpcmp_solve_batch_device": "pi" + "p" * 10, "mpcmp_warm_start_batch": "pippppp",
    # per-problem final-time windows and bounds
    "mpcmp_set_time_windows": "pipp", "mpcmp_set_time_windows_device": "pippp",
    "mpcmp_bounds_from_config": "pp", "mpcmp_bounds_from_margins": "dddddp", "mpcmp_set_bounds": "pip", "mpcmp_set_bounds_device": "pipp",
    # time scaling, time-synchronised solve
    "mpcmp_time_scale_batch": "pi" + "p" * 9, "mpcmp_time_scale_batch_device": "pi" + "p" * 10,
    "mpcmp_solve_batch_synced": "pi" + "p" * 6 + "i" + "p" * 5, "mpcmp_solve_batch_synced_device": "pi" + "p" * 6 + "i" + "p" * 6,
    # leaf kernels, resampling
    "mpcmp_rnea_batch": "pipppp", "mpcmp_eval_constraints_batch": "pipppp", "mpcmp_qp_batch": "pi" + "p" * 8,
    "mpcmp_sample_batch": "pipppip", "mpcmp_sample_batch_device": "pipppipp",
    # jerk-limited warm start
    "mpcmp_warm_start_jerk_batch": "pipppppp", "mpcmp_warm_start_jerk_batch_device": "pippppppp",
    "mpcmp_jerk_trajectory_batch": "pipppipp", "mpcmp_jerk_point_batch": "pipppppp",
    "mpcmp_warm_start_jerk_acc_batch": "pi" + "p" * 8, "mpcmp_warm_start_jerk_acc_batch_device": "pi" + "p" * 9,
    "mpcmp_jerk_trajectory_acc_batch": "pipppppipp", "mpcmp_jerk_point_acc_batch": "pi" + "p" * 8,
    "mpcmp_warm_start_jerk_lim_batch": "pi" + "p" * 10, "mpcmp_jerk_trajectory_lim_batch": "pi" + "p" * 7 + "ipp",
    "mpcmp_jerk_point_lim_batch": "pi" + "p" * 10, "mpcmp_mpc_point_batch": "pippppp",
    # scenario helpers of the robot wrapper
    "mpcmp_tool_jacobian": "ppppp", "mpcmp_forward_velocities": "pppp", "mpcmp_inverse_velocities": "ppppp", "mpcmp_inverse_kinematics": "pppppp",
    # batched tool-pose targets, trajectory checks
    "mpcmp_pose_targets_batch": "piipppipppp", "mpcmp_pose_targets_batch_device": "piipppippppp", "mpcmp_traj_stats_batch": "pippppip",
    # clearance
    "mpcmp_link_spheres": "pddipp", "mpcmp_clearance_config": "pippipipppp", "mpcmp_set_robot_spheres": "piip",
    "mpcmp_set_obstacles": "piip", "mpcmp_set_obstacles_device": "piipp",
    "mpcmp_clearance_batch": "pippidip", "mpcmp_clearance_batch_device": "pippidipp",
    "mpcmp_select_clear_batch": "pippppip", "mpcmp_select_clear_batch_device": "pippppipp",
    # via-point routes
    "mpcmp_route_via_velocity": "ppppidp", "mpcmp_route_legs": "pii" + "p" * 8, "mpcmp_route_legs_device": "pii" + "p" * 9,
    "mpcmp_route_join": "pii" + "p" * 9, "mpcmp_route_join_device": "pii" + "p" * 10,
    "mpcmp_solve_route_batch": "pii" + "p" * 14, "mpcmp_solve_route_batch_device": "pii" + "p" * 15,
    "mpcmp_route_locate": "ipdpp", "mpcmp_sample_route_batch": "piipppip", "mpcmp_sample_route_batch_device": "piipppipp",
    # receding-horizon driver
    "mpcmp_rh_init": "pipp", "mpcmp_rh_run": "pidi", "mpcmp_rh_get": "pppppp", "mpcmp_rh_stats": "ppp",
    "mpcmp_rh_update": "pipppi", "mpcmp_rh_update_device": "pipppip",
    # measurement hooks, diagnostics
    "mpcmp_kernel_timing": "pippp", "mpcmp_debug_fetch": "pipl", "mpcmp_debug_stamps": "pip",
}
# ... and every function include/mpcmp_limits.h declares (the between-node limit checker; mpcmp.h includes that header), in its order: the same
# rules, checked the same way by the CPU test suite
ABI_LIMITS = {
    "mpcmp_limits_batch": "pipppipp", "mpcmp_limits_batch_device": "pipppippp", "mpcmp_limits_config": "pi" + "p" * 8,
    "mpcmp_select_checked_batch": "pippppipip", "mpcmp_select_checked_batch_device": "pippppipipp",
}
# ... and every function include/mpcmp_retime.h declares (retiming of finished plans), in its order
ABI_RETIME = {
    "mpcmp_retime_batch": "pipppippp", "mpcmp_retime_batch_device": "pipppipppp", "mpcmp_retime_one": "piippppdipp",
    "mpcmp_sample_retimed_batch": "pipppipip", "mpcmp_sample_retimed_batch_device": "pipppipipp",
}
# ... and every function include/mpcmp_route_retime.h declares (retiming of whole routes), in its order
ABI_ROUTE_RETIME = {
    "mpcmp_retime_route_batch": "piipppipppp", "mpcmp_retime_route_batch_device": "piipppippppp", "mpcmp_retime_route_one": "piiipppppippp",
    "mpcmp_sample_retimed_route_batch": "piipppipip", "mpcmp_sample_retimed_route_batch_device": "piipppipipp",
}
# ... and every function include/mpcmp_retimed_check.h declares (limits of retimed plans and routes, profile scaling), in its order
ABI_RETIMED_CHECK = {
    "mpcmp_limits_retimed_batch": "pipppipippp", "mpcmp_limits_retimed_batch_device": "pipppipipppp",
    "mpcmp_limits_retimed_route_batch": "piipppipippp", "mpcmp_limits_retimed_route_batch_device": "piipppipipppp",
    "mpcmp_limits_retimed_one": "piiipppppipipp", "mpcmp_profile_scale_batch": "piipp", "mpcmp_profile_scale_batch_device": "piippp",
}
# ... and every function include/mpcmp_toolpath.h declares (tool-line moves), in its order
ABI_TOOLPATH = {
    "mpcmp_tool_line_batch": "pii" + "p" * 9, "mpcmp_tool_line_batch_device": "pii" + "p" * 10, "mpcmp_tool_line_one": "pipppppdpppp",
    "mpcmp_tool_deviation_batch": "piipppiddp", "mpcmp_tool_deviation_batch_device": "piipppiddpp", "mpcmp_tool_deviation_one": "pipppiddp",
}
# ... and every function include/mpcmp_clearance_cert.h declares (certified clearance), in its order
ABI_CLEARANCE_CERT = {
    "mpcmp_clearance_certified_batch": "pippdiiipp", "mpcmp_clearance_certified_batch_device": "pippdiiippp",
    "mpcmp_clearance_certified_one": "piippippddiiipp",
}
# ... and every function include/mpcmp_moving.h declares (clearance in a moving world), in its order
ABI_MOVING = {
    "mpcmp_set_obstacle_tracks": "piipiiddp", "mpcmp_set_obstacle_tracks_device": "piipiiddpp",
    "mpcmp_clearance_timed_batch": "pippippidip", "mpcmp_clearance_timed_batch_device": "pippippidipp",
    "mpcmp_start_delay_batch": "pippipipiidipp", "mpcmp_start_delay_batch_device": "pippipipiidippp",
    "mpcmp_sphere_tracks_batch": "pippippddip", "mpcmp_sphere_tracks_batch_device": "pippippddipp",
    "mpcmp_track_offset": "iddpdp", "mpcmp_clearance_timed_one": "piippipp" + "iiddp" + "pdipd" + "idip",
    "mpcmp_start_delay_one": "piippipp" + "iiddp" + "pdip" + "ipi" + "idi" + "pp",
}
# ... and every function include/mpcmp_moving_cert.h declares (certified clearance in a moving world), in its order
ABI_MOVING_CERT = {
    "mpcmp_clearance_certified_timed_batch": "pipppppdiiiipp", "mpcmp_clearance_certified_timed_batch_device": "pipppppdiiiippp",
    "mpcmp_clearance_certified_timed_one": "piippipp" + "iiddp" + "pdddd" + "diiii" + "pp",
}
# ... and every function include/mpcmp_field.h declares (voxel worlds: clearance against a distance field built on the GPU), in its order
ABI_FIELD = {
    "mpcmp_field_edt": "ppp", "mpcmp_field_sd": "ppppp", "mpcmp_clearance_field_config": "pipppppppp",
    "mpcmp_set_field": "ppp", "mpcmp_set_field_device": "pppp", "mpcmp_set_field_points": "ppip", "mpcmp_set_field_points_device": "ppipp",
    "mpcmp_get_field": "ppp", "mpcmp_clearance_field_batch": "pippidp", "mpcmp_clearance_field_batch_device": "pippidpp",
    "mpcmp_clearance_merge_batch": "pipppp", "mpcmp_clearance_merge_batch_device": "pippppp",
}
# ... and every function include/mpcmp_field_cert.h declares (certified clearance against a voxel world, the certificate merge), in its order
ABI_FIELD_CERT = {
    "mpcmp_clearance_certified_field_batch": "pippdiipp", "mpcmp_clearance_certified_field_batch_device": "pippdiippp",
    "mpcmp_clearance_certified_field_one": "piipppppddiipp",
    "mpcmp_clearance_cert_merge_batch": "pippp", "mpcmp_clearance_cert_merge_batch_device": "pipppp",
}
# ... and every function include/mpcmp_frame.h declares (camera frames as voxel worlds: the robot removed from clouds, depth images and grids), in
# its order
ABI_FRAME = {
    "mpcmp_frame_spheres": "pipppdp", "mpcmp_frame_points_one": "pipppipp" + "dipp", "mpcmp_frame_depth_one": "pippppp" + "ipdipp",
    "mpcmp_frame_carve_one": "pippppdpp",
    "mpcmp_set_field_points_filtered": "ppippdip", "mpcmp_set_field_points_filtered_device": "ppippdipp",
    "mpcmp_set_field_depth": "ppppipdip", "mpcmp_set_field_depth_device": "ppppipdipp",
    "mpcmp_field_carve": "ppdp", "mpcmp_field_carve_device": "ppdpp",
}
_KINDS = {"p": C.c_void_p, "i": C.c_int, "d": C.c_double, "l": C.c_long}
_RETURNS_TEXT = ("mpcmp_version", "mpcmp_last_error")         # const char *; every other function returns int
SYMBOLS = list(ABI)


def library_path():
    return _SO


def build_dependencies():
    """every file the library is built from, taken from the directories themselves: csrc/*.hip, csrc/*.cpp, csrc/*.hpp, csrc/Makefile and the C headers
    include/mpcmp*.h (mpcmp.h and what it includes; the C++ shim is a .hpp the library does not read)"""
    import glob
    src = os.path.join(_HERE, "csrc")
    deps = sorted(glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.cpp")) + glob.glob(os.path.join(src, "*.hpp")))
    return deps + [os.path.join(src, "Makefile")] + sorted(glob.glob(os.path.join(os.path.dirname(_HERE), "include", "mpcmp*.h")))


def build_library(force=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    deps = build_dependencies()
    if force or not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["make", "-C", src, "-B"], stdout=subprocess.DEVNULL)
    return _SO


_lib = None


def _torch_runtime_first():
    """torch bundles its own libamdhip64.so; libmpcmp.so links the system one (/opt/rocm), same soname.  Whichever is mapped first serves
    both: with torch's first everything works (the order bench.py and the tests have); with the system runtime first, a LATER `import torch`
    maps a second HIP runtime and reports "No HIP GPUs are available".  So: if torch is installed and not yet imported, import it before the
    library is loaded (MPCMP_NO_TORCH_PRELOAD=1 skips this, e.g. for torch-free deployments that want the shorter start-up)."""
    import sys
    if "torch" in sys.modules or os.environ.get("MPCMP_NO_TORCH_PRELOAD"):
        return
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        try:
            import torch  # noqa: F401
        except Exception as e:      # (say so — the system HIP runtime is mapped first now, and a later `import torch` would find no GPU)
            import warnings
            warnings.warn("mpc_motion_planner_amd: importing torch before loading libmpcmp.so failed (%r); a later `import torch` in this process "
                          "may report no GPU.  Set MPCMP_NO_TORCH_PRELOAD=1 to skip the preload." % (e,))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise MpcmpError(-2, "libmpcmp.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                                 "there is no CPU fallback" % _SO)
        _torch_runtime_first()
        L = C.CDLL(_SO)
        for name, kinds in list(ABI.items()) + list(ABI_LIMITS.items()) + list(ABI_RETIME.items()) + list(ABI_ROUTE_RETIME.items()) + list(ABI_RETIMED_CHECK.items()) + list(ABI_TOOLPATH.items()) + list(ABI_CLEARANCE_CERT.items()) + list(ABI_MOVING.items()) + list(ABI_MOVING_CERT.items()) + list(ABI_FIELD.items()) + list(ABI_FIELD_CERT.items()) + list(ABI_FRAME.items()):
            f = getattr(L, name)
            f.argtypes = [_KINDS[k] for k in kinds]
            f.restype = C.c_char_p if name in _RETURNS_TEXT else C.c_int
        _lib = L
    return _lib


def check(rc, ctx=None):
    if rc != 0:
        msg = lib().mpcmp_last_error(ctx)
        raise MpcmpError(rc, (msg or b"").decode())


def host(a):
    """the address of a host array for a pointer argument; None (NULL) for None and for an array without elements"""
    return a.ctypes.data if a is not None and a.size else None


def f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def default_model():
    m = Model(); check(lib().mpcmp_default_model(C.byref(m))); return m


def arm_models(bases, model=None):
    """ctypes array of Models for a multi-arm robot: `model` (default: the compiled-in Panda) mounted at every base =
    (yaw about world z, [x, y, z]); the base placement is folded into the first joint placement."""
    arr = (Model * len(bases))()
    for a, (yaw, xyz) in enumerate(bases):
        m = Model.from_buffer_copy(model if model is not None else default_model())
        c, s = np.cos(yaw), np.sin(yaw)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        R0 = Rz @ np.array(m.R0[0][:]).reshape(3, 3); p0 = np.asarray(xyz, dtype=np.float64) + Rz @ np.array(m.p[0][:])
        for i in range(9):
            m.R0[0][i] = R0.ravel()[i]
        for i in range(3):
            m.p[0][i] = p0[i]
        arr[a] = m
    return arr


DUAL_BASES = ((0.0, (0.0, 0.0, 0.0)), (np.pi, (1.0, 0.0, 0.0)))      # two Pandas facing each other, 1 m apart (configs[3] stand-in)


def payload(mass, com=(0.0, 0.0, 0.0), inertia=None):
    """a Payload from a mass, a COM [3] and a rotational inertia about the COM [3, 3] (default 0), all in the joint-7 frame"""
    p = Payload(); p.mass = float(mass)
    c = f64(com).reshape(3); I = np.zeros(9) if inertia is None else f64(inertia).reshape(9)
    for d in range(3):
        p.com[d] = c[d]
    for q in range(9):
        p.I[q] = I[q]
    return p


def model_add_payload(model, p):
    """mpcmp_model_add_payload: a copy of `model` with the Payload `p` lumped into body 7 (parallel-axis theorem)"""
    out = Model(); check(lib().mpcmp_model_add_payload(C.byref(model), C.byref(p), C.byref(out))); return out


def spheres(joint, c, r):
    """SPHERE_DTYPE records from joint [n], centres c [n][3] (in the joint's frame) and radii r (scalar or [n])"""
    joint = np.asarray(joint, dtype=np.int32).reshape(-1)
    t = np.zeros(joint.shape[0], dtype=SPHERE_DTYPE)
    t["joint"] = joint; t["c"] = f64(c).reshape(-1, 3); t["r"] = r
    return t


def obstacle(kind, a, b=(0.0, 0.0, 0.0), r=0.0):
    """one OBSTACLE_DTYPE record: OBS_SPHERE (a centre, r), OBS_CAPSULE (a..b, r), OBS_BOX (a centre, b half extents, r rounding),
    OBS_HALFSPACE (a unit normal into free space, b[0] offset: solid where a.x <= b[0])"""
    t = np.zeros((), dtype=OBSTACLE_DTYPE)
    t["type"] = kind; t["a"] = f64(a).reshape(3); t["b"] = f64(b).reshape(3); t["r"] = r
    return t


def _records(a, dtype, what):
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        raise ValueError("%s must be an array of %s records" % (what, what.upper() + "_DTYPE"))
    return a


def link_spheres(model, radius, spacing, max_spheres=MAX_SPHERES):
    """mpcmp_link_spheres: a SKELETON sphere model from the joint origins alone (not a fitted hull), SPHERE_DTYPE [n]"""
    out = np.zeros(max(int(max_spheres), 1), dtype=SPHERE_DTYPE); n = C.c_int(0)
    check(lib().mpcmp_link_spheres(C.byref(model), float(radius), float(spacing), int(max_spheres), host(out), C.byref(n)))
    return out[:n.value].copy()


def clearance_config(models, spheres_per_arm, obstacles, q, self_gap=0):
    """mpcmp_clearance_config: minimum clearance of ONE configuration q [7 narm] on the host.  models: a Model or a sequence of them;
    spheres_per_arm: one SPHERE_DTYPE array per arm; obstacles: OBSTACLE_DTYPE [n_obs] or None.  Returns (d_min, sphere, other)."""
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models)
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    obs = np.zeros(0, dtype=OBSTACLE_DTYPE) if obstacles is None else _records(obstacles, OBSTACLE_DTYPE, "obstacle").reshape(-1)
    q = f64(q).reshape(7 * narm)
    d, sp, ot = C.c_double(0), C.c_int(0), C.c_int(0)
    check(lib().mpcmp_clearance_config(arr, narm, host(cnt), host(tab), obs.shape[0], host(obs), int(self_gap), host(q), C.byref(d), C.byref(sp),
                                       C.byref(ot)))
    return d.value, sp.value, ot.value


def clearance_certified_one(models, num_seg, spheres_per_arm, obstacles, x, T, margin=0.0, self_gap=0, n_start=4, max_depth=10):
    """mpcmp_clearance_certified_one: the certified check of ONE plan x [N][14 narm] of duration T on the host (no context, no GPU).  models,
    spheres_per_arm and obstacles as for clearance_config.  Returns (the CLEARANCE_DTYPE record, the CLEARANCE_CERT_DTYPE record)."""
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    obs = np.zeros(0, dtype=OBSTACLE_DTYPE) if obstacles is None else _records(obstacles, OBSTACLE_DTYPE, "obstacle").reshape(-1)
    x = f64(x).reshape(N, 14 * narm)
    rec, cert = np.zeros(1, dtype=CLEARANCE_DTYPE), np.zeros(1, dtype=CLEARANCE_CERT_DTYPE)
    check(lib().mpcmp_clearance_certified_one(arr, narm, int(num_seg), host(cnt), host(tab), obs.shape[0], host(obs), host(x), float(T), float(margin),
                                              int(self_gap), int(n_start), int(max_depth), host(rec), host(cert)))
    return rec[0], cert[0]


def track_offset(P, t0, dt, tau):
    """mpcmp_track_offset: the offset [3] of the track P [n_key][3] on the clock t0 + k dt at world time tau (include/mpcmp_moving.h)"""
    P = f64(P).reshape(-1, 3); out = np.zeros(3)
    check(lib().mpcmp_track_offset(P.shape[0], float(t0), float(dt), host(P), float(tau), host(out)))
    return out


def _moving_one_args(models, num_seg, spheres_per_arm, obstacles, tracks, x):
    """the leading arguments mpcmp_clearance_timed_one and mpcmp_start_delay_one share; tracks: None or (track_of [n_obs], offsets
    [n_tracks][n_key][3], t0, dt).  Returns (the argument list through x, the arrays it points into)"""
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    obs = np.zeros(0, dtype=OBSTACLE_DTYPE) if obstacles is None else _records(obstacles, OBSTACLE_DTYPE, "obstacle").reshape(-1)
    if tracks is None:
        tof, off, n_tracks, n_key, t0, dt = np.zeros(0, dtype=np.int32), np.zeros(0), 0, 1, 0.0, 1.0
    else:
        tof = np.ascontiguousarray(tracks[0], dtype=np.int32).reshape(-1); off = f64(tracks[1])
        if off.ndim != 3 or off.shape[2] != 3 or tof.shape[0] != obs.shape[0]:
            raise ValueError("tracks: track_of [n_obs] and offsets [n_tracks][n_key][3]")
        n_tracks, n_key, t0, dt = off.shape[0], off.shape[1], float(tracks[2]), float(tracks[3])
    x = f64(x).reshape(N, 14 * narm)
    keep = (arr, cnt, tab, obs, tof, off, x)
    return [arr, narm, int(num_seg), host(cnt), host(tab), obs.shape[0], host(obs), host(tof), n_tracks, n_key, t0, dt, host(off), host(x)], keep


def _profile_arg(prof):
    if prof is None:
        return 0, None, None
    prof = f64(prof)
    if prof.ndim != 2 or prof.shape[1] != 2 or prof.shape[0] < 2:
        raise ValueError("prof must be [n_grid + 1][2]")
    return prof.shape[0] - 1, host(prof), prof


def clearance_timed_one(models, num_seg, spheres_per_arm, obstacles, tracks, x, T, prof=None, t_start=0.0, n_pts=200, margin=0.0, self_gap=0):
    """mpcmp_clearance_timed_one: the timed check of ONE plan x [N][14 narm] of duration T on the host (no context, no GPU) in the world `obstacles`
    moved by tracks = (track_of, offsets [n_tracks][n_key][3], t0, dt) or None; prof [n_grid + 1][2] or None.  Returns the CLEARANCE_DTYPE record"""
    args, keep = _moving_one_args(models, num_seg, spheres_per_arm, obstacles, tracks, x)
    n_grid, pp, keep2 = _profile_arg(prof)
    rec = np.zeros(1, dtype=CLEARANCE_DTYPE)
    check(lib().mpcmp_clearance_timed_one(*args, float(T), n_grid, pp, float(t_start), int(n_pts), float(margin), int(self_gap), host(rec)))
    return rec[0]


def start_delay_one(models, num_seg, spheres_per_arm, obstacles, tracks, x, T, delays, prof=None, check_wait=False, n_pts=200, margin=0.0, self_gap=0):
    """mpcmp_start_delay_one: the start-delay search of ONE plan on the host.  Returns (the START_DELAY_DTYPE record, d_min_all [K])"""
    args, keep = _moving_one_args(models, num_seg, spheres_per_arm, obstacles, tracks, x)
    n_grid, pp, keep2 = _profile_arg(prof)
    delays = f64(delays).reshape(-1)
    rec, d_all = np.zeros(1, dtype=START_DELAY_DTYPE), np.zeros(max(delays.shape[0], 1))
    check(lib().mpcmp_start_delay_one(*args, float(T), n_grid, pp, delays.shape[0], host(delays), int(bool(check_wait)), int(n_pts), float(margin),
                                      int(self_gap), host(d_all), host(rec)))
    return rec[0], d_all[:delays.shape[0]]


def clearance_certified_timed_one(models, num_seg, spheres_per_arm, obstacles, tracks, x, T, t_start=0.0, wait_before=0.0, hold_after=0.0, margin=0.0,
                                  self_gap=0, n_start=4, n_rest=4, max_depth=10):
    """mpcmp_clearance_certified_timed_one: the certified check of ONE plan x [N][14 narm] of duration T in the moving world (tracks as for
    clearance_timed_one), the motion starting at the world time t_start after a wait of wait_before at the first posture and followed by a hold of
    hold_after at the last, on the host (no context, no GPU).  Returns (the CLEARANCE_DTYPE record, the CLEARANCE_CERT_DTYPE record); times are on
    the record clock, which starts with the wait (include/mpcmp_moving_cert.h)"""
    args, keep = _moving_one_args(models, num_seg, spheres_per_arm, obstacles, tracks, x)
    rec, cert = np.zeros(1, dtype=CLEARANCE_DTYPE), np.zeros(1, dtype=CLEARANCE_CERT_DTYPE)
    check(lib().mpcmp_clearance_certified_timed_one(*args, float(T), float(t_start), float(wait_before), float(hold_after), float(margin), int(self_gap),
                                                    int(n_start), int(n_rest), int(max_depth), host(rec), host(cert)))
    return rec[0], cert[0]


def field_desc(origin, h, n):
    """one FIELD_DESC_DTYPE record: the grid of n = (n0, n1, n2) cubes of edge h whose lowest corner is `origin` (world frame); voxel (i, j, k) has
    the linear index (k n1 + j) n0 + i, so an occupancy array is indexed occ[k][j][i]"""
    t = np.zeros((), dtype=FIELD_DESC_DTYPE)
    t["origin"] = f64(origin).reshape(3); t["h"] = float(h); t["n"] = np.asarray(n, dtype=np.int32).reshape(3)
    return t


def _field_desc_arg(desc):
    desc = np.ascontiguousarray(desc).reshape(())
    if desc.dtype != FIELD_DESC_DTYPE:
        raise ValueError("desc must be one FIELD_DESC_DTYPE record (field_desc)")
    return desc


def _field_array(desc, a, dtype, what):
    """a [n2][n1][n0] (or flat) as a contiguous array of `dtype` with the voxel count of desc"""
    n = [int(v) for v in desc["n"]]
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size != n[0] * n[1] * n[2]:
        raise ValueError("%s must hold n2 x n1 x n0 = %d x %d x %d entries, got %s" % (what, n[2], n[1], n[0], a.shape))
    return a.reshape(n[2], n[1], n[0])


def field_edt(desc, occ):
    """mpcmp_field_edt: the exact squared distance field d2 [n2][n1][n0] (uint32, voxel units, FIELD_EMPTY everywhere when nothing is occupied) of
    the occupancy occ [n2][n1][n0] (nonzero: solid) on the host (no GPU)"""
    desc = _field_desc_arg(desc)
    occ = _field_array(desc, np.asarray(occ) != 0, np.uint8, "occ")
    d2 = np.zeros(occ.shape, dtype=np.uint32)
    check(lib().mpcmp_field_edt(desc.ctypes.data, host(occ), host(d2)))
    return d2


def field_sd(desc, d2, x):
    """mpcmp_field_sd: (sd_field(x), the linear index of the voxel read) for the world point x [3] (include/mpcmp_field.h, "Distance")"""
    desc = _field_desc_arg(desc); d2 = _field_array(desc, d2, np.uint32, "d2"); x = f64(x).reshape(3)
    sd, v = C.c_double(0), C.c_int(0)
    check(lib().mpcmp_field_sd(desc.ctypes.data, host(d2), host(x), C.byref(sd), C.byref(v)))
    return sd.value, v.value


def clearance_field_config(models, spheres_per_arm, desc, d2, q):
    """mpcmp_clearance_field_config: minimum field clearance of ONE configuration q [7 narm] on the host; models and spheres_per_arm as for
    clearance_config.  Returns (d_min, sphere, voxel)."""
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models)
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    desc = _field_desc_arg(desc); d2 = _field_array(desc, d2, np.uint32, "d2")
    q = f64(q).reshape(7 * narm)
    d, sp, vx = C.c_double(0), C.c_int(0), C.c_int(0)
    check(lib().mpcmp_clearance_field_config(arr, narm, host(cnt), host(tab), desc.ctypes.data, host(d2), host(q), C.byref(d), C.byref(sp),
                                             C.byref(vx)))
    return d.value, sp.value, vx.value


def clearance_certified_field_one(models, num_seg, spheres_per_arm, desc, d2, x, T, margin=0.0, n_start=4, max_depth=10):
    """mpcmp_clearance_certified_field_one: the certified check of ONE plan x [N][14 narm] of duration T against the field d2 of the grid desc on the
    host (no context, no GPU).  models and spheres_per_arm as for clearance_config, desc and d2 as for field_sd.  Returns (the CLEARANCE_DTYPE
    record, the CLEARANCE_CERT_DTYPE record)."""
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    desc = _field_desc_arg(desc); d2 = _field_array(desc, d2, np.uint32, "d2")
    x = f64(x).reshape(N, 14 * narm)
    rec, cert = np.zeros(1, dtype=CLEARANCE_DTYPE), np.zeros(1, dtype=CLEARANCE_CERT_DTYPE)
    check(lib().mpcmp_clearance_certified_field_one(arr, narm, int(num_seg), host(cnt), host(tab), desc.ctypes.data, host(d2), host(x), float(T),
                                                    float(margin), int(n_start), int(max_depth), host(rec), host(cert)))
    return rec[0], cert[0]


def camera(R, t, fx, fy, cx, cy, width, height, depth_scale=1.0, z_min=0.0, z_max=np.inf):
    """one CAMERA_DTYPE record (mpcmp_camera): R [3][3] and t [3] map the camera frame to the world frame, pixel (row v, column u) of depth d lies at
    z = d depth_scale, p = (z (u - cx) / fx, z (v - cy) / fy, z); pixels with z outside [z_min, z_max] are invalid.  z_max must be finite for the
    library (the default here is for the reader's convenience: pass the sensor's range)"""
    c = np.zeros((), dtype=CAMERA_DTYPE)
    c["R"] = f64(R).reshape(9); c["t"] = f64(t).reshape(3)
    c["fx"], c["fy"], c["cx"], c["cy"] = float(fx), float(fy), float(cx), float(cy)
    c["depth_scale"], c["z_min"], c["z_max"] = float(depth_scale), float(z_min), float(z_max)
    c["width"], c["height"] = int(width), int(height)
    return c


def _camera_arg(cam):
    cam = np.ascontiguousarray(cam).reshape(())
    if cam.dtype != CAMERA_DTYPE:
        raise ValueError("camera must be one CAMERA_DTYPE record (capi.camera)")
    return cam


def _depth_arg(cam, depth):
    """(the image as a contiguous uint16 or float32 array of the camera's size, its depth type)"""
    depth = np.asarray(depth)
    if depth.dtype != np.uint16:
        depth = depth.astype(np.float32, copy=False)
    depth = np.ascontiguousarray(depth)
    if depth.size != int(cam["width"]) * int(cam["height"]):
        raise ValueError("depth must hold height x width = %d x %d entries, got %s" % (cam["height"], cam["width"], depth.shape))
    return depth, (DEPTH_U16 if depth.dtype == np.uint16 else DEPTH_F32)


def _frame_robot(models, spheres_per_arm, q):
    """(the Model array, narm, the counts, the table, q or None) of the host statements of include/mpcmp_frame.h; with q None no robot is read"""
    if q is None:
        return None, 1, None, None, None
    if isinstance(models, Model):
        models = [models]; spheres_per_arm = [spheres_per_arm] if isinstance(spheres_per_arm, np.ndarray) else spheres_per_arm
    narm = len(models)
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    per = [_records(sp, SPHERE_DTYPE, "sphere").reshape(-1) for sp in spheres_per_arm]
    if len(per) != narm:
        raise ValueError("one sphere table per arm")
    cnt = np.array([p.shape[0] for p in per], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(per)) if per else np.zeros(0, dtype=SPHERE_DTYPE)
    return arr, narm, cnt, tab, f64(q).reshape(7 * narm)


def _frame_occ(desc, occ, keep):
    n = [int(v) for v in desc["n"]]
    if occ is None:
        if keep:
            raise ValueError("keep needs the occupancy to add to")
        return np.zeros((n[2], n[1], n[0]), dtype=np.uint8)
    return _field_array(desc, (np.asarray(occ) != 0).astype(np.uint8), np.uint8, "occ").copy()


def frame_spheres(models, spheres_per_arm, q, pad):
    """mpcmp_frame_spheres: the filter spheres [ns][4] = world centre, r + pad of the posture q [7 narm] on the host"""
    arr, narm, cnt, tab, q = _frame_robot(models, spheres_per_arm, f64(q))
    out = np.zeros((tab.shape[0], 4))
    check(lib().mpcmp_frame_spheres(arr, narm, host(cnt), host(tab), host(q), float(pad), host(out) if out.size else out.ctypes.data))
    return out


def frame_points_one(models, spheres_per_arm, desc, points, q, pad, keep=False, occ=None):
    """mpcmp_frame_points_one: (occ [n2][n1][n0] uint8, the FRAME_STATS_DTYPE record) of the cloud points [n][3] with the robot at q [7 narm] (None:
    no filter) removed, on the host; keep: marked into a copy of `occ`"""
    arr, narm, cnt, tab, q = _frame_robot(models, spheres_per_arm, q)
    desc = _field_desc_arg(desc); pts = f64(points).reshape(-1, 3); occ = _frame_occ(desc, occ, keep)
    st = np.zeros((), dtype=FRAME_STATS_DTYPE)
    check(lib().mpcmp_frame_points_one(arr, narm, host(cnt) if cnt is not None else None, host(tab) if tab is not None else None, desc.ctypes.data,
                                       pts.shape[0], host(pts), host(q) if q is not None else None, float(pad), FRAME_KEEP if keep else 0,
                                       occ.ctypes.data, st.ctypes.data))
    return occ, st


def frame_depth_one(models, spheres_per_arm, desc, cam, depth, q, pad, keep=False, occ=None):
    """mpcmp_frame_depth_one: the same for a depth image depth [height][width] (uint16, or anything else as float32) of the camera cam"""
    arr, narm, cnt, tab, q = _frame_robot(models, spheres_per_arm, q)
    desc = _field_desc_arg(desc); cam = _camera_arg(cam); depth, kind = _depth_arg(cam, depth); occ = _frame_occ(desc, occ, keep)
    st = np.zeros((), dtype=FRAME_STATS_DTYPE)
    check(lib().mpcmp_frame_depth_one(arr, narm, host(cnt) if cnt is not None else None, host(tab) if tab is not None else None, desc.ctypes.data,
                                      cam.ctypes.data, depth.ctypes.data, kind, host(q) if q is not None else None, float(pad),
                                      FRAME_KEEP if keep else 0, occ.ctypes.data, st.ctypes.data))
    return occ, st


def frame_carve_one(models, spheres_per_arm, desc, occ, q, pad):
    """mpcmp_frame_carve_one: (a copy of occ with the robot at q carved out, the FRAME_STATS_DTYPE record) on the host"""
    arr, narm, cnt, tab, q = _frame_robot(models, spheres_per_arm, q)
    desc = _field_desc_arg(desc); occ = _frame_occ(desc, occ, True)
    st = np.zeros((), dtype=FRAME_STATS_DTYPE)
    check(lib().mpcmp_frame_carve_one(arr, narm, host(cnt) if cnt is not None else None, host(tab) if tab is not None else None, desc.ctypes.data,
                                      host(q) if q is not None else None, float(pad), occ.ctypes.data, st.ctypes.data))
    return occ, st


def limits_spec(tol=None, tool_lin_max=np.inf, tool_ang_max=np.inf):
    """one LIMITS_SPEC_DTYPE record: tol a scalar or [7] (default 0), the tool speed maxima (default +inf: no such limit)"""
    t = np.zeros((), dtype=LIMITS_SPEC_DTYPE)
    t["tol"] = 0.0 if tol is None else np.broadcast_to(f64(tol), (7,))
    t["tool_lin_max"] = tool_lin_max; t["tool_ang_max"] = tool_ang_max
    return t


def limits_config(models, row, q, qd, qdd, spec=None):
    """mpcmp_limits_config: ONE configuration q, qd, qdd [7 narm] on the host under the BOUNDS_DTYPE record `row` and the LIMITS_SPEC_DTYPE record
    `spec` (None: tol 0, no tool limits).  models: a Model or a sequence of them.  Returns (excess [7], channel [7], ratios [4] = r_v, r_a, r_lin,
    r_ang)."""
    if isinstance(models, Model):
        models = [models]
    narm = len(models)
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    row = np.ascontiguousarray(row).reshape(())
    if row.dtype != BOUNDS_DTYPE:
        raise ValueError("row must be one BOUNDS_DTYPE record")
    if spec is not None:
        spec = np.ascontiguousarray(spec).reshape(())
        if spec.dtype != LIMITS_SPEC_DTYPE:
            raise ValueError("spec must be one LIMITS_SPEC_DTYPE record")
    q, qd, qdd = [f64(v).reshape(7 * narm) for v in (q, qd, qdd)]
    ex, ch, r = np.zeros(7), np.zeros(7, dtype=np.int32), np.zeros(4)
    check(lib().mpcmp_limits_config(arr, narm, host(row), None if spec is None else spec.ctypes.data, host(q), host(qd), host(qdd), host(ex),
                                    host(ch), host(r)))
    return ex, ch, r


def retime_spec(tool_lin_max=np.inf, tool_ang_max=np.inf, rate_max=1.0, groups=RT_ALL_GROUPS):
    """one RETIME_SPEC_DTYPE record: the tool speed maxima (default +inf: none), the largest rate (default 1: never faster than the plan) and the
    mask of the groups that take part (bits 1 << LIM_QD, LIM_QDD, LIM_TAU, LIM_TOOL_LIN, LIM_TOOL_ANG)"""
    t = np.zeros((), dtype=RETIME_SPEC_DTYPE)
    t["tool_lin_max"] = tool_lin_max; t["tool_ang_max"] = tool_ang_max; t["rate_max"] = rate_max; t["groups"] = groups
    return t


def _retime_spec_arg(spec):
    if spec is None:
        return None
    spec = np.ascontiguousarray(spec).reshape(())
    if spec.dtype != RETIME_SPEC_DTYPE:
        raise ValueError("spec must be one RETIME_SPEC_DTYPE record")
    return spec


def retime_one(models, num_seg, row, x, u, T, n_grid=200, spec=None):
    """mpcmp_retime_one: ONE trajectory x [N][14 narm], u [N][7 narm], T on the host (no context, no GPU) under the BOUNDS_DTYPE record `row` and the
    RETIME_SPEC_DTYPE record `spec` (None: no tool limits, rate_max 1, all groups).  models: a Model or a sequence of them.  Returns
    (prof [n_grid + 1][2] = (t_k, x_k), the RETIME_DTYPE record)."""
    if isinstance(models, Model):
        models = [models]
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    row = np.ascontiguousarray(row).reshape(())
    if row.dtype != BOUNDS_DTYPE:
        raise ValueError("row must be one BOUNDS_DTYPE record")
    spec = _retime_spec_arg(spec)
    x, u = f64(x).reshape(N, 14 * narm), f64(u).reshape(N, 7 * narm)
    prof = np.zeros((max(int(n_grid), 0) + 1, 2)); rec = np.zeros(1, dtype=RETIME_DTYPE)
    check(lib().mpcmp_retime_one(arr, narm, int(num_seg), host(row), None if spec is None else spec.ctypes.data, host(x), host(u), float(T), int(n_grid),
                                 host(prof), host(rec)))
    return prof, rec[0]


def retime_route_one(models, num_seg, rows, x, u, T, n_grid=200, spec=None):
    """mpcmp_retime_route_one: ONE route of n_legs legs x [n_legs][N][14 narm], u [n_legs][N][7 narm], T [n_legs] on the host (no context, no GPU), leg
    m under the BOUNDS_DTYPE record rows[m] (one record: every leg under it) and the RETIME_SPEC_DTYPE record `spec` (None: no tool limits, rate_max
    1, all groups).  models: a Model or a sequence of them, for every leg.  Returns (prof [n_legs][n_grid + 1][2] = (t_k, x_k) with leg times,
    leg_T_new [n_legs], the ROUTE_RETIME_DTYPE record)."""
    if isinstance(models, Model):
        models = [models]
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    T = f64(T).reshape(-1); nl = T.shape[0]
    rows = np.ascontiguousarray(rows)
    if rows.dtype != BOUNDS_DTYPE:
        raise ValueError("rows must be BOUNDS_DTYPE records")
    rows = np.ascontiguousarray(np.broadcast_to(rows.reshape(-1), (nl,))) if rows.size == 1 else rows.reshape(-1)
    if rows.shape[0] != nl:
        raise ValueError("one BOUNDS_DTYPE record per leg (or one for all): %d legs, %d rows" % (nl, rows.shape[0]))
    spec = _retime_spec_arg(spec)
    x, u = f64(x).reshape(nl, N, 14 * narm), f64(u).reshape(nl, N, 7 * narm)
    prof = np.zeros((nl, max(int(n_grid), 0) + 1, 2)); leg_T = np.zeros(nl); rec = np.zeros(1, dtype=ROUTE_RETIME_DTYPE)
    check(lib().mpcmp_retime_route_one(arr, narm, int(num_seg), nl, host(rows), None if spec is None else spec.ctypes.data, host(x), host(u), host(T),
                                       int(n_grid), host(prof), host(leg_T), host(rec)))
    return prof, leg_T, rec[0]


def limits_retimed_one(models, num_seg, rows, x, u, T, prof, n_pts=200, spec=None):
    """mpcmp_limits_retimed_one: the limit record of ONE retimed plan or route on the host (no context, no GPU): n_legs legs x [n_legs][N][14 narm],
    u [n_legs][N][7 narm], T [n_legs] (a plan: one leg, the leading axis may be left out), leg m under the BOUNDS_DTYPE record rows[m] (one record:
    every leg under it), prof [n_legs][n_grid + 1][2] as retime_one / retime_route_one left it, the LIMITS_SPEC_DTYPE record `spec` (None: tol 0, no
    tool limits).  models: a Model or a sequence of them, for every leg.  Returns (the LIMITS_DTYPE record, T_new)."""
    if isinstance(models, Model):
        models = [models]
    narm = len(models); N = 3 * int(num_seg) + 1
    arr = (Model * narm)(*[Model.from_buffer_copy(m) for m in models])
    T = f64(T).reshape(-1); nl = T.shape[0]
    rows = np.ascontiguousarray(rows)
    if rows.dtype != BOUNDS_DTYPE:
        raise ValueError("rows must be BOUNDS_DTYPE records")
    rows = np.ascontiguousarray(np.broadcast_to(rows.reshape(-1), (nl,))) if rows.size == 1 else rows.reshape(-1)
    if rows.shape[0] != nl:
        raise ValueError("one BOUNDS_DTYPE record per leg (or one for all): %d legs, %d rows" % (nl, rows.shape[0]))
    if spec is not None:
        spec = np.ascontiguousarray(spec).reshape(())
        if spec.dtype != LIMITS_SPEC_DTYPE:
            raise ValueError("spec must be one LIMITS_SPEC_DTYPE record")
    x, u = f64(x).reshape(nl, N, 14 * narm), f64(u).reshape(nl, N, 7 * narm)
    prof = f64(prof)
    if prof.ndim < 2 or prof.shape[-1] != 2 or prof.size % (2 * nl) or prof.size < 4 * nl:
        raise ValueError("prof must be [n_legs][n_grid + 1][2] with n_legs = %d" % nl)
    prof = prof.reshape(nl, -1, 2)
    rec = np.zeros(1, dtype=LIMITS_DTYPE); T_new = np.zeros(1)
    check(lib().mpcmp_limits_retimed_one(arr, narm, int(num_seg), nl, host(rows), None if spec is None else spec.ctypes.data, host(x), host(u), host(T),
                                         prof.shape[1] - 1, host(prof), int(n_pts), host(rec), host(T_new)))
    return rec[0], float(T_new[0])


def tool_line_spec(tool_lin_max=1.7, tool_ang_max=2.5, T_min=0.2, damp=1e-8, manip_min=1e-3, eps=1e-9, n_sub=4):
    """one TOOL_LINE_SPEC_DTYPE record; the defaults are those of a NULL spec (include/mpcmp_toolpath.h)"""
    t = np.zeros((), dtype=TOOL_LINE_SPEC_DTYPE)
    t["tool_lin_max"] = tool_lin_max; t["tool_ang_max"] = tool_ang_max; t["T_min"] = T_min; t["damp"] = damp; t["manip_min"] = manip_min
    t["eps"] = eps; t["n_sub"] = n_sub
    return t


def _tool_line_spec_arg(spec):
    if spec is None:
        return None
    spec = np.ascontiguousarray(spec).reshape(())
    if spec.dtype != TOOL_LINE_SPEC_DTYPE:
        raise ValueError("spec must be one TOOL_LINE_SPEC_DTYPE record")
    return spec


def tool_line_one(model, num_seg, row, q_start, R1, p1, T=0.0, spec=None):
    """mpcmp_tool_line_one: ONE straight tool line of one arm on the host (no context, no GPU) from the posture q_start [7] to the pose R1 [3][3],
    p1 [3], as a plan under the position rows of the BOUNDS_DTYPE record `row`; T <= 0: the duration rule.  Returns (x [N][14], u [N][7], T, the
    TOOL_LINE_DTYPE record)."""
    N = 3 * int(num_seg) + 1
    row = np.ascontiguousarray(row).reshape(())
    if row.dtype != BOUNDS_DTYPE:
        raise ValueError("row must be one BOUNDS_DTYPE record")
    spec = _tool_line_spec_arg(spec)
    q, R1, p1 = f64(q_start).reshape(7), f64(R1).reshape(9), f64(p1).reshape(3)
    x, u, To, rec = np.zeros((N, 14)), np.zeros((N, 7)), np.zeros(1), np.zeros(1, dtype=TOOL_LINE_DTYPE)
    check(lib().mpcmp_tool_line_one(C.byref(model), int(num_seg), host(row), None if spec is None else spec.ctypes.data, host(q), host(R1), host(p1),
                                    float(T), host(x), host(u), host(To), host(rec)))
    return x, u, float(To[0]), rec[0]


def tool_deviation_one(model, num_seg, x, R1, p1, n_pts=200, tol_lin=np.inf, tol_ang=np.inf):
    """mpcmp_tool_deviation_one: the TOOL_DEV_DTYPE record of ONE plan x [N][14] of one arm against the line from the tool pose of its node 0 to
    R1, p1 (host, no GPU)"""
    N = 3 * int(num_seg) + 1
    x, R1, p1 = f64(x).reshape(N, 14), f64(R1).reshape(9), f64(p1).reshape(3)
    rec = np.zeros(1, dtype=TOOL_DEV_DTYPE)
    check(lib().mpcmp_tool_deviation_one(C.byref(model), int(num_seg), host(x), host(R1), host(p1), int(n_pts), float(tol_lin), float(tol_ang),
                                         host(rec)))
    return rec[0]


def model_from_urdf(path):
    m = Model(); check(lib().mpcmp_model_from_urdf(path.encode(), C.byref(m))); return m


def models_from_urdf(path, max_chains=8):
    """Every serial 7-joint chain of the URDF (file order) as a ctypes array of Models, ready for Solver(models=...):
    fixed joints, base placements, rotated inertial frames and joint axes other than +z are folded in (mpcmp.h)."""
    arr = (Model * max_chains)(); n = C.c_int(0)
    check(lib().mpcmp_models_from_urdf(path.encode(), max_chains, arr, C.byref(n)))
    out = (Model * n.value)()
    for i in range(n.value):
        out[i] = arr[i]
    return out


# ---- scenario helpers of the robot wrapper (host side; robot_utils/pandaWrapper.cpp:14-107) ----
def tool_jacobian(model, q):
    """World-aligned 6x7 tool-frame Jacobian [linear; angular], tool position and rotation."""
    q = f64(q); J = np.zeros((6, 7)); p = np.zeros(3); R = np.zeros((3, 3))
    check(lib().mpcmp_tool_jacobian(C.byref(model), host(q), host(J), host(p), host(R)))
    return J, p, R


def forward_velocities(model, q, qd):
    """PandaWrapper::forward_velocities: task velocity [linear(3); angular(3)] of the tool frame."""
    q, qd = f64(q), f64(qd); out = np.zeros(6)
    check(lib().mpcmp_forward_velocities(C.byref(model), host(q), host(qd), host(out)))
    return out


def inverse_velocities(model, q, linear_velocity, angular_velocity):
    """PandaWrapper::inverse_velocities: damped (1e-5) pseudo-inverse map from task to joint velocity."""
    q, lin, ang = f64(q), f64(linear_velocity), f64(angular_velocity); out = np.zeros(7)
    check(lib().mpcmp_inverse_velocities(C.byref(model), host(q), host(lin), host(ang), host(out)))
    return out


def inverse_kinematic(model, orientation, position, q_init=None):
    """PandaWrapper::inverse_kinematic: returns (q, converged, iterations); the start configuration is explicit."""
    R, p = f64(orientation), f64(position); q = np.zeros(7); it = C.c_int(0)
    qi = f64(q_init) if q_init is not None else None
    rc = lib().mpcmp_inverse_kinematics(C.byref(model), host(R), host(p), host(qi), host(q), C.byref(it))
    if rc not in (0, 1):
        check(rc)
    return q, rc == 0, it.value


def default_limits():
    out = [np.zeros(7) for _ in range(6)]
    check(lib().mpcmp_default_limits(*[host(o) for o in out]))
    return dict(zip(["qmin", "qmax", "vmax", "amax", "jmax", "taumax"], out))


def default_config(num_seg=4, sqp_iters=20, margins=None, **kw):
    c = Config(); check(lib().mpcmp_default_config(C.byref(c), int(num_seg), int(sqp_iters)))
    if margins is not None:
        check(lib().mpcmp_set_margins(C.byref(c), *[float(x) for x in margins[:4]]))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def bounds_from_config(cfg):
    """mpcmp_bounds_from_config: the six bound tables of a Config as one BOUNDS_DTYPE record (bit for bit)"""
    out = np.zeros((), dtype=BOUNDS_DTYPE)
    check(lib().mpcmp_bounds_from_config(C.byref(cfg), host(out)))
    return out


def bounds_from_margins(margin_position=1.0, margin_velocity=1.0, margin_acceleration=1.0, margin_torque=1.0, min_height=0.05):
    """mpcmp_bounds_from_margins: the tables of default_config + mpcmp_set_margins + mpcmp_set_min_height as one BOUNDS_DTYPE record"""
    out = np.zeros((), dtype=BOUNDS_DTYPE)
    check(lib().mpcmp_bounds_from_margins(float(margin_position), float(margin_velocity), float(margin_acceleration), float(margin_torque),
                                          float(min_height), host(out)))
    return out


def route_via_velocity(p_prev, p_via, p_next, row, narm=1, speed=1.0):
    """mpcmp_route_via_velocity: the chord rule's pass-through velocity [7 narm] at p_via between p_prev and p_next, within the limits of the
    BOUNDS_DTYPE record `row` (host, no GPU)"""
    a, b, c = [f64(v).reshape(7 * narm) for v in (p_prev, p_via, p_next)]
    row = np.ascontiguousarray(row).reshape(())
    if row.dtype != BOUNDS_DTYPE:
        raise ValueError("row must be one BOUNDS_DTYPE record")
    v = np.zeros(7 * narm)
    check(lib().mpcmp_route_via_velocity(host(a), host(b), host(c), host(row), int(narm), float(speed), host(v)))
    return v


def route_locate(leg_T, t):
    """mpcmp_route_locate: (leg, normalised time) of the route time t on the legs of durations leg_T (host, no GPU)"""
    T = f64(leg_T).reshape(-1); leg, tau = C.c_int(0), C.c_double(0)
    check(lib().mpcmp_route_locate(T.shape[0], host(T), float(t), C.byref(leg), C.byref(tau)))
    return leg.value, tau.value


def num_nodes(num_seg):
    return lib().mpcmp_num_nodes(int(num_seg))


def time_nodes(num_seg):
    t = np.zeros(3 * num_seg + 1); check(lib().mpcmp_time_nodes(int(num_seg), host(t))); return t
