"""mpc_motion_planner_amd — host-side binding of libmpcmp.so (HIP / gfx950).

The product is the C-ABI shared library declared in include/mpcmp.h; this module is the thin ctypes
binding used by bench.py and the parity tests, plus `BatchMotionPlanner`, a batched mirror of the
reference's `MotionPlanner` façade (mpc_solver/motionPlanner.hpp:16-176).  There is no CPU fallback:
loading fails loudly when the HIP library is missing, and every solver call fails when no GPU is present.
(The scenario helpers of the robot wrapper — Jacobian, velocity maps, inverse kinematics — are host code in the
reference and here; they are not part of the batched solve.  Their batched form for targets, `Solver.pose_targets`, runs
multi-start inverse kinematics on the GPU.)
"""
from .capi import (STATUS_NAN, STATUS_NOT_PD, STATUS_XCH_DEAD, STATUS_QP_CAPPED, STATUS_OUTSIDE_TOL, STATUS_T_OUT_OF_BOX, STATUS_ARRIVED, STATUS_HARD,
                   RH_RESTART, IK_NOT_CONVERGED, IK_Q_OUT_OF_BOUNDS, IK_QD_OUT_OF_BOUNDS, IK_INFO_DTYPE, Config, Info, Model, Payload, INFO_DTYPE, MpcmpError, DUAL_BASES, arm_models, build_library, default_config, default_limits,
                   default_model, forward_velocities, inverse_kinematic, inverse_velocities, lib, library_path,
                   model_add_payload, model_from_urdf, models_from_urdf, num_nodes, payload, time_nodes, tool_jacobian,
                   SPHERE_DTYPE, OBSTACLE_DTYPE, CLEARANCE_DTYPE, OBS_SPHERE, OBS_CAPSULE, OBS_BOX, OBS_HALFSPACE, CLR_HIT, CLR_NAN,
                   CLR_UNDECIDED, CLEARANCE_CERT_DTYPE, clearance_certified_one, clearance_certified_timed_one,
                   START_DELAY_DTYPE, MAX_TRACKS, MAX_TRACK_KEYS, MAX_DELAYS, track_offset, clearance_timed_one, start_delay_one,
                   FIELD_DESC_DTYPE, FIELD_EMPTY, FIELD_MAX_DIM, FIELD_MAX_VOXELS, field_desc, field_edt, field_sd, clearance_field_config,
                   CAMERA_DTYPE, FRAME_STATS_DTYPE, DEPTH_U16, DEPTH_F32, FRAME_KEEP, FRAME_MAX_PIXELS, camera, frame_spheres, frame_points_one,
                   frame_depth_one, frame_carve_one,
                   clearance_certified_field_one,
                   spheres, obstacle, link_spheres, clearance_config, BOUNDS_DTYPE, bounds_from_config, bounds_from_margins,
                   ROUTE_SEAM_DTYPE, route_via_velocity, route_locate,
                   LIMITS_SPEC_DTYPE, LIMITS_DTYPE, LIM_GROUPS, LIM_Q, LIM_QD, LIM_QDD, LIM_TAU, LIM_HEIGHT, LIM_TOOL_LIN, LIM_TOOL_ANG, LIM_NAN, limits_spec, limits_config,
                   RETIME_SPEC_DTYPE, RETIME_DTYPE, RT_INFEASIBLE, RT_NAN, RT_ALL_GROUPS, retime_spec, retime_one,
                   ROUTE_RETIME_DTYPE, retime_route_one, limits_retimed_one,
                   TOOL_LINE_SPEC_DTYPE, TOOL_LINE_DTYPE, TOOL_DEV_DTYPE, TL_STOPPED, TL_Q_OUT_OF_BOUNDS, TD_OVER, TL_NAN, tool_line_spec, tool_line_one,
                   tool_deviation_one)
from .planner import BatchMotionPlanner, Solver

__all__ = ["TOOL_LINE_SPEC_DTYPE", "TOOL_LINE_DTYPE", "TOOL_DEV_DTYPE", "TL_STOPPED", "TL_Q_OUT_OF_BOUNDS", "TD_OVER", "TL_NAN", "tool_line_spec",
           "tool_line_one", "tool_deviation_one",
           "STATUS_NAN", "STATUS_NOT_PD", "STATUS_XCH_DEAD", "STATUS_QP_CAPPED", "STATUS_OUTSIDE_TOL", "STATUS_T_OUT_OF_BOX", "STATUS_ARRIVED", "STATUS_HARD", "RH_RESTART",
           "IK_NOT_CONVERGED", "IK_Q_OUT_OF_BOUNDS", "IK_QD_OUT_OF_BOUNDS", "IK_INFO_DTYPE",
           "Config", "Info", "Model", "INFO_DTYPE", "MpcmpError", "build_library", "default_config",
           "default_limits", "default_model", "lib", "library_path", "model_from_urdf", "models_from_urdf", "num_nodes",
           "time_nodes", "BatchMotionPlanner", "Solver", "forward_velocities", "inverse_kinematic",
           "inverse_velocities", "tool_jacobian", "arm_models", "DUAL_BASES", "Payload", "payload", "model_add_payload",
           "SPHERE_DTYPE", "OBSTACLE_DTYPE", "CLEARANCE_DTYPE", "OBS_SPHERE", "OBS_CAPSULE", "OBS_BOX", "OBS_HALFSPACE", "CLR_HIT", "CLR_NAN",
           "CLR_UNDECIDED", "CLEARANCE_CERT_DTYPE", "clearance_certified_one", "clearance_certified_timed_one",
           "START_DELAY_DTYPE", "MAX_TRACKS", "MAX_TRACK_KEYS", "MAX_DELAYS", "track_offset", "clearance_timed_one", "start_delay_one",
           "spheres", "obstacle", "link_spheres", "clearance_config",
           "FIELD_DESC_DTYPE", "FIELD_EMPTY", "FIELD_MAX_DIM", "FIELD_MAX_VOXELS", "field_desc", "field_edt", "field_sd", "clearance_field_config",
           "CAMERA_DTYPE", "FRAME_STATS_DTYPE", "DEPTH_U16", "DEPTH_F32", "FRAME_KEEP", "FRAME_MAX_PIXELS", "camera", "frame_spheres", "frame_points_one",
           "frame_depth_one", "frame_carve_one",
           "clearance_certified_field_one",
           "BOUNDS_DTYPE", "bounds_from_config", "bounds_from_margins",
           "ROUTE_SEAM_DTYPE", "route_via_velocity", "route_locate",
           "LIMITS_SPEC_DTYPE", "LIMITS_DTYPE", "LIM_GROUPS", "LIM_Q", "LIM_QD", "LIM_QDD", "LIM_TAU", "LIM_HEIGHT", "LIM_TOOL_LIN", "LIM_TOOL_ANG", "LIM_NAN", "limits_spec", "limits_config",
           "RETIME_SPEC_DTYPE", "RETIME_DTYPE", "RT_INFEASIBLE", "RT_NAN", "RT_ALL_GROUPS", "retime_spec", "retime_one",
           "ROUTE_RETIME_DTYPE", "retime_route_one", "limits_retimed_one"]
