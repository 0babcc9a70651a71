"""ctypes binding of ``libparc_env.so`` (C-ABI in ``include/parc_env.h``).

There is no CPU fallback: if the HIP library is missing or fails to load, importing the env raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PARC_ENV_LIB: developer override used to A/B kernel builds; the shipped library is the in-tree one
LIB_PATH = os.environ.get("PARC_ENV_LIB") or os.path.join(_HERE, "libparc_env.so")

ABI_VERSION = 6
MAX_BODIES, MAX_DOFS, MAX_TAR_STEPS, MAX_KEY, MAX_FK_PATHS, MAX_FK_DEPTH, MAX_GEOMS = 16, 40, 6, 8, 8, 8, 24

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)


class ParcCharModel(C.Structure):
    _fields_ = [("num_bodies", C.c_int32), ("dof_size", C.c_int32), ("parent", C.c_int32 * MAX_BODIES),
                ("local_translation", (C.c_float * 3) * MAX_BODIES), ("local_rotation", (C.c_float * 4) * MAX_BODIES),
                ("joint_type", C.c_int32 * MAX_BODIES), ("joint_axis", (C.c_float * 3) * MAX_BODIES),
                ("dof_idx", C.c_int32 * MAX_BODIES), ("fk_paths", (C.c_int32 * MAX_FK_DEPTH) * MAX_FK_PATHS)]


class ParcDynamicsParams(C.Structure):
    _fields_ = [("num_geoms", C.c_int32), ("geom_body", C.c_int32 * MAX_GEOMS), ("geom_type", C.c_int32 * MAX_GEOMS),
                ("geom_pos", (C.c_float * 3) * MAX_GEOMS), ("geom_pos2", (C.c_float * 3) * MAX_GEOMS),
                ("geom_size", (C.c_float * 3) * MAX_GEOMS), ("geom_density", C.c_float * MAX_GEOMS),
                ("dof_stiffness", C.c_float * MAX_DOFS), ("dof_damping", C.c_float * MAX_DOFS),
                ("dof_armature", C.c_float * MAX_DOFS), ("dof_effort", C.c_float * MAX_DOFS),
                ("dof_lower", C.c_float * MAX_DOFS), ("dof_upper", C.c_float * MAX_DOFS),
                ("gravity_z", C.c_float), ("sim_dt", C.c_float), ("sim_steps", C.c_int32), ("substeps", C.c_int32),
                ("solver_iterations", C.c_int32), ("friction", C.c_float), ("restitution", C.c_float),
                ("contact_offset", C.c_float), ("max_depenetration_velocity", C.c_float),
                ("angular_damping", C.c_float), ("max_angular_velocity", C.c_float), ("control_mode", C.c_int32)]


class ParcEnvConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("struct_size", C.c_uint32), ("device", C.c_int32), ("num_envs", C.c_int32),
                ("model", ParcCharModel), ("num_key_bodies", C.c_int32), ("key_body_ids", C.c_int32 * MAX_KEY),
                ("num_tar_obs_steps", C.c_int32), ("tar_obs_steps", C.c_int32 * MAX_TAR_STEPS),
                ("num_rays", C.c_int32), ("ray_points_host", f32p), ("control_dt", C.c_double),
                ("episode_length", C.c_float), ("min_obs_h", C.c_float), ("max_obs_h", C.c_float),
                ("pose_w", C.c_float), ("vel_w", C.c_float), ("root_pos_w", C.c_float), ("root_vel_w", C.c_float),
                ("key_pos_w", C.c_float), ("joint_err_w", C.c_float * MAX_BODIES), ("dof_err_w", C.c_float * MAX_DOFS),
                ("contact_weights", C.c_float * MAX_BODIES), ("pose_termination_dist", C.c_float * MAX_BODIES),
                ("root_pos_termination_dist", C.c_float), ("root_rot_termination_angle", C.c_float),
                ("enable_early_termination", C.c_int32), ("pose_termination", C.c_int32), ("track_root", C.c_int32),
                ("track_root_h", C.c_int32), ("report_tracking_error", C.c_int32),
                ("fail_rate_ema_weight", C.c_float), ("min_motion_weight", C.c_float),
                ("rand_root_pos_offset_scale", C.c_float), ("rand_reset", C.c_int32), ("demo_mode", C.c_int32),
                ("env_offsets_host", f32p), ("action_low", C.c_float * MAX_DOFS), ("action_high", C.c_float * MAX_DOFS),
                ("body_pos_from_fk", C.c_int32), ("enable_dynamics", C.c_int32), ("dynamics", ParcDynamicsParams),
                ("seed", C.c_uint64), ("contact_body_mask", C.c_uint32), ("termination_height", C.c_float),
                ("global_obs", C.c_int32), ("global_root_height_obs", C.c_int32),
                ("use_contact_info", C.c_int32), ("enable_tar_obs", C.c_int32), ("dev_options", C.c_char_p)]


class ParcMotionClips(C.Structure):
    _fields_ = [("num_motions", C.c_int32), ("num_frames_host", i32p), ("fps_host", i32p), ("loop_modes_host", i32p),
                ("weights_host", f64p), ("root_pos_host", f32p), ("root_rot_host", f32p), ("joint_rot_host", f32p),
                ("contacts_host", f32p)]


CAMERA_TRACK, CAMERA_STILL = 0, 1   # PARC_CAMERA_*


class ParcRenderParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("camera_mode", C.c_int32),
                ("offset", C.c_float * 3), ("eye", C.c_float * 3), ("target", C.c_float * 3), ("fov_y", C.c_float),
                ("sun_dir", C.c_float * 3), ("ref_offset", C.c_float * 3),
                ("draw_ref", C.c_int32), ("shadows", C.c_int32), ("debug_visuals", C.c_int32)]


MOPT_NUM_TERMS, MOPT_MAX_POINTS = 9, 512   # PARC_MOPT_*


class ParcMotionOptParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("num_points", C.c_int32),
                ("points_host", f32p), ("point_body_host", i32p), ("geom0_type", C.c_int32 * MAX_BODIES),
                ("geom0_offset", (C.c_float * 3) * MAX_BODIES), ("geom0_radius", C.c_float * MAX_BODIES),
                ("contact_body_id", C.c_int32 * MAX_BODIES), ("weights", C.c_float * 9), ("max_jerk", C.c_float),
                ("step_size", C.c_float)]


MTERR_SDF_PRUNED, MTERR_SDF_BRUTE = 0, 1   # PARC_MTERR_SDF_*
MTERR_CLIP_OUTPUTS = 6


class ParcMotionTerrainParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("num_points", C.c_int32),
                ("points_host", f32p), ("point_body_host", i32p), ("contact_body_id", C.c_int32 * MAX_BODIES),
                ("z_buf", C.c_double), ("jump_buf", C.c_double), ("max_jerk", C.c_double), ("sdf_mode", C.c_int32)]


MEDIT_MAX_FRAMES, MEDIT_FLAG_WORDS = 4096, 64   # PARC_MEDIT_*


class ParcMotionEditParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("hesitation_val", C.c_float),
                ("hesitation_min_seq_len", C.c_int32)]


MLABEL_MAX_FOOT_BOXES = 8   # PARC_MLABEL_*


class ParcMotionLabelParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("foot_body", C.c_int32 * 2),
                ("hand_body", C.c_int32 * 2), ("hand_radius", C.c_float * 2), ("num_foot_boxes", C.c_int32),
                ("box_foot", C.c_int32 * MLABEL_MAX_FOOT_BOXES), ("box_offset", (C.c_float * 3) * MLABEL_MAX_FOOT_BOXES),
                ("box_half", (C.c_float * 3) * MLABEL_MAX_FOOT_BOXES), ("contact_eps", C.c_float)]


class ParcMotionOptClips(C.Structure):
    _fields_ = [("num_clips", C.c_int32), ("frame_off_host", i64p), ("hf_off_host", i64p), ("cons_off_host", i64p),
                ("hf_dims_host", i32p), ("hf_geom_host", f32p), ("hf_host", f32p), ("root_pos_host", f32p), ("root_rot_host", f32p),
                ("joint_rot_host", f32p), ("contacts_host", f32p), ("cons_body_host", i32p), ("cons_range_host", i32p),
                ("cons_point_host", f32p)]


MSAMP_MAX_FRAMES, MSAMP_MAX_GRID, MSAMP_MAX_TERRAIN_CELLS, MSAMP_MAX_BOXES, MSAMP_BOX_FLOATS = 64, 32, 512 * 512, 64, 6   # PARC_MSAMP_*
MSAMP_RELATIVE_Z = {"RELATIVE_TO_ROOT": 0, "RELATIVE_TO_ROOT_FLOOR": 1}                               # PARC_MSAMP_RELATIVE_TO_*
MSAMP_AUG_MODE = {"NOISE": 0, "MAXPOOL_AND_BOXES": 1, "NONE": 2}                                    # PARC_MSAMP_AUG_*
MSAMP_POOL_NONE, MSAMP_POOL_2D, MSAMP_POOL_1D_X, MSAMP_POOL_1D_Y = 0, 1, 2, 3                       # PARC_MSAMP_POOL_*
MSAMP_STATUS = {1: "motion_id outside the library", 2: "num_boxes outside [0, max_num_boxes]", 4: "pool kind or size out of range"}


class ParcMotionSamplerParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("num_frames", C.c_int32),
                ("times_host", f32p), ("timestep", C.c_float), ("sequence_duration", C.c_float), ("ref_frame", C.c_int32),
                ("autoregressive", C.c_int32), ("relative_z_style", C.c_int32), ("aug_mode", C.c_int32),
                ("grid_dim_x", C.c_int32), ("grid_dim_y", C.c_int32), ("num_x_neg", C.c_int32), ("num_y_neg", C.c_int32),
                ("grid_x_host", f32p), ("grid_y_host", f32p), ("grid_min_x", C.c_float), ("grid_min_y", C.c_float),
                ("dx", C.c_float), ("max_h", C.c_float), ("max_num_boxes", C.c_int32), ("box_min_len", C.c_float),
                ("box_max_len", C.c_float), ("hf_maxpool_chance", C.c_float), ("hf_max_maxpool_size", C.c_int32),
                ("hf_change_height_chance", C.c_float), ("future_pos_noise_scale", C.c_float),
                ("future_window_min", C.c_float), ("future_window_max", C.c_float)]


class ParcMotionSamplerClipInfo(C.Structure):
    _fields_ = [("hf_maxmin_host", f32p), ("mask_off_host", i64p), ("mask_cells_host", i32p), ("fps_host", i32p),
                ("loop_modes_host", i32p), ("weights_host", f64p)]


# (field, dtype, per-sample shape in terms of max_num_boxes mb / grid gx, gy): the plan's device arrays, in struct order
MSAMP_PLAN_FIELDS = [("motion_id", "i", ()), ("t0", "f", ()), ("t_future", "f", ()), ("future_pos_noise", "f", (3,)),
                     ("change_height", "i", ()), ("height_value", "f", ()), ("pool_kind", "i", (3,)), ("pool_size", "i", (3,)),
                     ("num_boxes", "i", ()), ("boxes", "f", ("mb", MSAMP_BOX_FLOATS)), ("noise", "f", ("gx", "gy"))]
MSAMP_OUTPUT_FIELDS = ["root_pos", "root_rot", "joint_pos", "joint_rot", "contacts", "floor_heights", "hfs", "target_pos", "target_rot",
                       "hf_bounds"]


class ParcMotionSamplerPlan(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(n, C.c_void_p) for n, _, _ in MSAMP_PLAN_FIELDS]


class ParcMotionSamplerOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MSAMP_OUTPUT_FIELDS]


PATHPLAN_MAX_DIM, PATHPLAN_MAX_JUMP_RADIUS, PATHPLAN_JUMP_WORDS = 64, 8, 8   # PARC_PATHPLAN_*
PATHPLAN_STATUS = ("FOUND", "NO_PATH", "OVER_MAX_COST", "BUDGET", "NO_DRAW")
PATHPLAN_SETTINGS = ("max_z_diff", "max_jump_xy_dist", "max_jump_z_diff", "min_jump_z_diff", "w_z", "w_xy", "w_bumpy", "max_bumpy",
                     "uniform_cost_max", "uniform_cost_min", "min_start_end_xy_dist", "max_cost")   # AStarSettings, in struct order
PATHPLAN_OUTPUT_FIELDS = [("status", "i"), ("cost", "f"), ("num_nodes", "i"), ("nodes", "i"), ("num_points", "i"), ("points", "f"),
                          ("start", "i"), ("goal", "i"), ("hf", "f"), ("pops", "i")]


class ParcPathPlanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("dim_x", C.c_int32), ("dim_y", C.c_int32), ("dx", C.c_float),
                ("dy", C.c_float), ("min_point", C.c_float * 2)] + [(n, C.c_double) for n in PATHPLAN_SETTINGS] + \
               [("simplify_terrain", C.c_int32), ("max_expansions", C.c_int32), ("max_nodes", C.c_int32), ("max_points", C.c_int32)]


class ParcPathPlanOutputs(C.Structure):
    _fields_ = [(n, {"f": f32p, "i": i32p}[t]) for n, t in PATHPLAN_OUTPUT_FIELDS]


TGEN_MAX_DIM, TGEN_MAX_BOXES, TGEN_MAX_PATHS, TGEN_MAX_STAIRS, TGEN_MAX_POOL = 64, 64, 64, 16, 8   # PARC_TGEN_*
TGEN_PATH_POINTS, TGEN_MAX_STEPS, TGEN_BOX_FLOATS, TGEN_STAIR_FLOATS = 1000, 1024, 6, 7
TGEN_MODES = ("BOXES", "PATHS", "STAIRS")                                                        # PARC_TGEN_BOXES / PATHS / STAIRS
# the three settings blocks, in struct order: (name, "i" / "f")
TGEN_BOXES_FIELDS = [("num_boxes", "i"), ("min_box_h", "f"), ("max_box_h", "f"), ("box_min_len", "f"), ("box_max_len", "f"),
                     ("min_box_angle", "f"), ("max_box_angle", "f")]
TGEN_PATHS_FIELDS = [("num_terrain_paths", "i"), ("maxpool_size", "i"), ("path_min_height", "f"), ("path_max_height", "f"), ("floor_height", "f")]
TGEN_STAIRS_FIELDS = [("num_stairs", "i"), ("min_stair_start_height", "f"), ("max_stair_start_height", "f"), ("min_step_height", "f"),
                      ("max_step_height", "f"), ("min_stair_thickness", "f"), ("max_stair_thickness", "f")]
TGEN_PLAN_FIELDS = ["boxes", "path_start", "path_vy", "path_angle", "path_turn", "path_height", "stairs"]


class ParcTerrainGenParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("mode", C.c_int32), ("dim_x", C.c_int32), ("dim_y", C.c_int32),
                ("dx", C.c_float), ("dy", C.c_float), ("min_point", C.c_float * 2)] + \
               [(n, C.c_int32 if t == "i" else C.c_float) for n, t in TGEN_BOXES_FIELDS + TGEN_PATHS_FIELDS + TGEN_STAIRS_FIELDS]


class ParcTerrainGenPlan(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(n, C.c_void_p) for n in TGEN_PLAN_FIELDS]


MAUG_MAX_DIM, MAUG_MAX_BOXES, MAUG_BOX_FLOATS = 128, 16, 4                                         # PARC_MAUG_*
MAUG_MODES = ("HEIGHT_SCALE", "BOXES_ALONG_PATH", "NONE")                                         # PARC_MAUG_HEIGHT_SCALE / BOXES_ALONG_PATH / NONE
MAUG_STATUS_CLAMPED, MAUG_STATUS_NOT_FINITE = 1, 2
# the plan's arrays, in struct order: (name, "i" / "f", per-variation shape)
MAUG_PLAN_FIELDS = [("src_clip", "i", ()), ("start_frame", "i", ()), ("num_frames", "i", ()), ("heading", "f", ()), ("scale", "f", (2,)),
                    ("mirror", "i", ()), ("height_scale", "f", ()), ("num_boxes", "i", ()), ("box_frame", "i", (MAUG_MAX_BOXES,)),
                    ("boxes", "f", (MAUG_MAX_BOXES, MAUG_BOX_FLOATS))]
MAUG_OUTPUT_FIELDS = ["frame_off", "cell_off", "src_clip", "hf_dims", "hf_geom", "canon_z", "root_pos", "root_rot", "joint_rot", "contacts",
                      "hf", "hf_maxmin"]


class ParcMotionAugParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel),
                ("joint_swap", C.c_int32 * MAX_BODIES), ("contact_swap", C.c_int32 * MAX_BODIES),
                ("mode", C.c_int32), ("terrain_padding_size", C.c_int32), ("slice_terrain", C.c_int32), ("sample_weight_by_length", C.c_int32),
                ("min_heading_angle", C.c_float), ("max_heading_angle", C.c_float), ("x_scale", C.c_float * 2), ("y_scale", C.c_float * 2),
                ("min_h_scale", C.c_float), ("max_h_scale", C.c_float), ("bad_h_range", C.c_float * 2),
                ("min_num_boxes", C.c_int32), ("max_num_boxes", C.c_int32),
                ("min_len", C.c_float), ("max_len", C.c_float), ("min_angle", C.c_float), ("max_angle", C.c_float),
                ("min_h", C.c_float), ("max_h", C.c_float)]


class ParcMotionAugClipInfo(C.Structure):
    _fields_ = [("hf_maxmin_host", f32p), ("fps_host", i32p), ("max_frames_host", i32p)]


class ParcMotionAugPlan(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(n, C.c_void_p) for n, _, _ in MAUG_PLAN_FIELDS]


class ParcMotionAugSizes(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_maxmin", C.c_int32), ("total_frames", C.c_int64), ("total_cells", C.c_int64)]


class ParcMotionAugOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MAUG_OUTPUT_FIELDS]


BUFFER_FIELDS = [
    ("char_root_pos", "f"), ("char_root_rot", "f"), ("char_root_vel", "f"), ("char_root_ang_vel", "f"),
    ("char_dof_pos", "f"), ("char_dof_vel", "f"), ("char_body_pos", "f"), ("contact_forces", "f"),
    ("motion_ids", "i"), ("terrain_ids", "i"), ("time_offsets", "f"), ("timestep", "i"), ("time", "f"), ("ep_num", "l"),
    ("obs", "f"), ("reward", "f"), ("done", "i"), ("reward_terms", "f"), ("tracking_error", "f"),
    ("ref_root_pos", "f"), ("ref_root_rot", "f"), ("ref_root_vel", "f"), ("ref_root_ang_vel", "f"),
    ("ref_joint_rot", "f"), ("ref_dof_pos", "f"), ("ref_dof_vel", "f"), ("ref_body_pos", "f"), ("ref_contacts", "f"),
    ("ray_hfs", "f"),
]


MDM_MAX_LAYERS, MDM_MAX_HIDDEN, MDM_MAX_WIDTH, MDM_MAX_DIM, MDM_MAX_SEQ, MDM_MAX_STEPS, MDM_GRID = 8, 8, 1024, 512, 64, 4096, 31   # PARC_MDM_*
MDM_DDIM, MDM_DDPM = 0, 1
MDM_PASS_PLAIN, MDM_PASS_GUIDED, MDM_PASS_UNCOND = 0, 1, 2


class ParcMdmParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel),
                ("d_model", C.c_int32), ("num_heads", C.c_int32), ("d_hid", C.c_int32), ("num_layers", C.c_int32),
                ("seq_len", C.c_int32), ("num_prev_states", C.c_int32), ("diffusion_timesteps", C.c_int32),
                ("frame_dim", C.c_int32), ("target_dim", C.c_int32),
                ("num_target_hidden", C.c_int32), ("num_in_hidden", C.c_int32), ("num_out_hidden", C.c_int32),
                ("target_hidden", C.c_int32 * MDM_MAX_HIDDEN), ("in_hidden", C.c_int32 * MDM_MAX_HIDDEN), ("out_hidden", C.c_int32 * MDM_MAX_HIDDEN),
                ("max_batch", C.c_int32), ("weights_host", f32p), ("weight_offsets_host", i64p), ("num_tensors", C.c_int32),
                ("mean_host", f32p), ("std_host", f32p), ("sqrt_alphas_cumprod_host", f32p), ("sqrt_one_minus_alphas_cumprod_host", f32p),
                ("posterior_mean_coef1_host", f32p), ("posterior_mean_coef2_host", f32p), ("posterior_std_host", f32p)]


class ParcMdmConds(C.Structure):
    _fields_ = [("n", C.c_int32), ("hf", C.c_void_p), ("target", C.c_void_p), ("prev_state", C.c_void_p), ("obs_flag", C.c_void_p),
                ("target_flag", C.c_void_p), ("prev_state_flag", C.c_void_p), ("noise_ind", C.c_void_p)]


class ParcMdmSampleArgs(C.Structure):
    _fields_ = [("mode", C.c_int32), ("num_steps", C.c_int32), ("timesteps_host", i32p), ("stride", C.c_int32), ("use_guidance", C.c_int32),
                ("guidance_scale", C.c_float), ("x", C.c_void_p), ("noise", C.c_void_p), ("draw", C.c_int32), ("seed", C.c_uint64),
                ("first_index", C.c_uint64), ("keep", C.c_void_p)]


MLOSS_NUM_TERMS, MLOSS_SQUARED_L2, MLOSS_PSEUDO_HUBER = 13, 0, 1   # PARC_MLOSS_*


class ParcMotionLossParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("model", ParcCharModel), ("sequence_fps", C.c_float),
                ("num_prev_states", C.c_int32), ("weights", C.c_float * MLOSS_NUM_TERMS), ("use_pos_loss", C.c_int32),
                ("use_target_loss", C.c_int32), ("target_dir_len_eps", C.c_float), ("loss_fn", C.c_int32)]


class ParcMotionLossArgs(C.Structure):
    _fields_ = [("n", C.c_int32), ("num_frames", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("pred", "mean", "std", "root_pos", "root_rot", "joint_rot", "contacts", "target_dir", "terms", "grad")]


MPATH_HEADING_AUTO, MPATH_HEADING_RANDOM = 0, 1   # PARC_MPATH_HEADING_*


class ParcMdmPathParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mdm", C.c_void_p), ("grid_dx", C.c_float), ("grid_dy", C.c_float),
                ("num_x_neg", C.c_int32), ("num_x_pos", C.c_int32), ("num_y_neg", C.c_int32), ("num_y_pos", C.c_int32),
                ("max_h", C.c_float), ("sequence_fps", C.c_float), ("left_foot", C.c_int32), ("right_foot", C.c_int32),
                ("next_node_lookahead", C.c_int32), ("rewind_num_frames", C.c_int32), ("max_motion_length", C.c_float),
                ("use_prev_state", C.c_int32), ("use_cfg", C.c_int32), ("cfg_scale", C.c_float), ("prev_state_ind_key", C.c_int32),
                ("target_condition_key", C.c_int32), ("use_ddim", C.c_int32), ("ddim_stride", C.c_int32)]


class ParcMdmPathCondOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("hf", "target", "prev_state", "obs_flag", "target_flag", "prev_state_flag", "noise_ind", "done",
                                          "closest_node", "target_node", "canon")]


class ParcMdmPathAppendArgs(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.c_void_p), ("prev_state", C.c_void_p), ("noise_ind", C.c_void_p), ("canon", C.c_void_p),
                ("guided", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("offset", C.c_int32), ("frames", C.c_void_p),
                ("max_frames", C.c_int32), ("prev_next", C.c_void_p), ("done", C.c_void_p), ("final_frame", C.c_void_p), ("total", C.c_int32)]


class ParcMdmPathRolloutArgs(C.Structure):
    _fields_ = [("prev_frames", C.c_void_p), ("rel_height_host", f32p), ("heading_host", f32p), ("heading_mode", C.c_int32),
                ("noise", C.c_void_p), ("noise_windows", C.c_int32), ("seed", C.c_uint64), ("row_ids_host", i64p), ("path_ids_host", i64p), ("frames", C.c_void_p),
                ("final_frame", C.c_void_p), ("done", C.c_void_p)]


MSEL_MAX_SLICE_DIM, MSEL_RUN_LAUNCHES = 1024, 4   # PARC_MSEL_*
MSEL_STATUS = {1: "a root position is not finite", 2: "a side of the slice exceeds PARC_MSEL_MAX_SLICE_DIM", 4: "the motion has no frame"}


class ParcPathSelectParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mpath", C.c_void_p), ("num_points", C.c_int32), ("points_host", f32p), ("point_body_host", i32p),
                ("contact_body_id", C.c_int32 * MAX_BODIES), ("w_contact", C.c_float), ("w_pen", C.c_float), ("not_finished_penalty", C.c_float),
                ("slice_padding", C.c_float), ("sdf_mode", C.c_int32)]


class ParcPathSelectArgs(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("num_frames", C.c_int32), ("frame_stride", C.c_int32), ("final_frame", C.c_void_p), ("noise", C.c_void_p),
                ("slice_terrain", C.c_int32), ("max_contact_loss", C.c_float), ("max_pen_loss", C.c_float), ("max_total_loss", C.c_float)]


class ParcPathSelectResults(C.Structure):
    _fields_ = [("contact_loss", f32p), ("pen_loss", f32p), ("total_loss", f32p), ("valid", i32p), ("status", i32p), ("num_frames", i32p),
                ("slice_min_point", f32p), ("slice_dims", i32p), ("order", i32p), ("num_valid", i32p)]


class ParcEnvBuffers(C.Structure):
    _fields_ = [(n, {"f": f32p, "i": i32p, "l": i64p}[t]) for n, t in BUFFER_FIELDS]


def _signatures():
    """``name -> (restype, argtypes)`` of every function ``include/parc_env.h`` declares, in the header's order and sections.  ``load()``
    applies it, and a name without a row fails the export check, so no function is left to ctypes' defaults by accident."""
    P = C.POINTER
    vp, i32, i64, u32, u64, f32, cstr = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_char_p
    rc = C.c_int   # the return code that check() reads (the counts that three getters return are ints too)
    u8p, u32p, u64p = P(C.c_uint8), P(u32), P(u64)
    plan_s, out_s = P(ParcMotionSamplerPlan), P(ParcMotionSamplerOutputs)
    return {
        # version
        "parc_last_error": (cstr, []),
        "parc_abi_version": (rc, []),
        # env: lifecycle, loads, buffers
        "parc_env_create": (rc, [P(ParcEnvConfig), P(vp)]),
        "parc_env_destroy": (None, [vp]),
        "parc_env_obs_dim": (rc, [vp]),
        "parc_env_load_motions": (rc, [vp, P(ParcMotionClips)]),
        "parc_env_load_terrain": (rc, [vp, f32p, i32, i32, f32, f32, f32, f32, f32p, i32, i32]),
        "parc_env_bind_buffers": (rc, [vp, P(ParcEnvBuffers)]),
        "parc_env_get_buffers": (rc, [vp, P(ParcEnvBuffers)]),
        # env: step and resets
        "parc_env_step": (rc, [vp, vp, vp]),
        "parc_env_reset": (rc, [vp, vp, i32, vp]),
        "parc_env_reset_with": (rc, [vp, vp, i32, vp, vp, vp, vp, vp]),
        "parc_env_reset_done": (rc, [vp, vp]),
        "parc_env_compute_obs": (rc, [vp, vp, i32, vp]),
        # env: curriculum and reset settings
        "parc_env_get_fail_rates": (rc, [vp, f32p, i32]),
        "parc_env_set_fail_rates": (rc, [vp, f32p, i32]),
        "parc_env_get_motion_info": (rc, [vp, f32p, f32p, i32]),
        "parc_env_set_never_done": (rc, [vp, i32]),
        "parc_env_set_rand_reset": (rc, [vp, i32, i32, f32]),
        "parc_env_set_start_time_fraction": (rc, [vp, vp]),
        # device ops on the env's character and motion library
        "parc_dof_to_rot": (rc, [vp, vp, vp, i32, vp]),
        "parc_rot_to_dof": (rc, [vp, vp, vp, i32, vp]),
        "parc_forward_kinematics": (rc, [vp, vp, vp, vp, vp, vp, i32, vp]),
        "parc_calc_motion_frame": (rc, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "parc_test_quat_op": (rc, [i32, vp, vp, vp, i32, vp, vp]),
        # build and diagnostics
        "parc_build_flags": (cstr, []),
        "parc_env_get_frame_vel_tables": (rc, [vp, f32p, f32p, f32p]),
        "parc_env_profile_step": (rc, [vp, vp, vp, i32, f32p, f32p]),
        "parc_env_describe": (cstr, [vp]),
        "parc_env_dynamics_timeouts": (rc, [vp]),
        "parc_env_health_words": (u32p, [vp]),
        "parc_env_dynamics_manifold_drops": (rc, [vp]),
        "parc_env_last_dynamics_ms": (f32, [vp]),
        "parc_env_set_episode_length": (rc, [vp, f32]),
        # captured step + reset
        "parc_env_bind_action": (rc, [vp, vp]),
        "parc_env_step_reset_graph": (rc, [vp, vp]),
        # learner kernels
        "parc_td_lambda_return": (rc, [vp, vp, vp, f32, f32, i32, i32, vp, vp]),
        "parc_normalize_record": (rc, [vp, vp, vp, f32, vp, vp, i64, i32, vp]),
        "parc_gather_rows": (rc, [i32, P(vp), P(vp), i64p, vp, i64, i64, vp]),
        # recording
        "parc_env_record_bind": (rc, [vp, vp, vp, i32, vp, vp, vp, i32]),
        "parc_env_record_frame": (rc, [vp, vp]),
        # kernel timing and kernel names
        "parc_env_set_kernel_timing": (rc, [vp, i32]),
        "parc_env_get_kernel_timing": (rc, [vp, f64p, f64p, P(i32)]),
        "parc_env_get_kernel_timing_samples": (rc, [vp, f32p, f32p, f32p, i32, P(i32)]),
        "parc_env_dynamics_kernel": (cstr, [vp]),
        "parc_env_post_kernel": (cstr, [vp]),
        # render
        "parc_env_render": (rc, [vp, P(ParcRenderParams), vp, i32, vp, vp, vp, vp]),
        "parc_env_render_scene": (rc, [vp, P(ParcRenderParams), i32, vp, i32, vp, vp, vp, vp, vp]),
        # motion optimiser
        "parc_mopt_create": (rc, [P(ParcMotionOptParams), P(vp)]),
        "parc_mopt_destroy": (None, [vp]),
        "parc_mopt_set_clips": (rc, [vp, P(ParcMotionOptClips)]),
        "parc_mopt_set_constraint_points": (rc, [vp, f32p]),
        "parc_mopt_set_params": (rc, [vp, f32p]),
        "parc_mopt_get_params": (rc, [vp, f32p]),
        "parc_mopt_loss_and_grad": (rc, [vp, f32p, f32p]),
        "parc_mopt_step": (rc, [vp, i32, f32p]),
        "parc_mopt_get_frames": (rc, [vp, f32p, f32p, f32p]),
        "parc_mopt_get_source_body": (rc, [vp, f32p, f32p]),
        "parc_mopt_build_constraints": (rc, [vp, i32, i32p, f32p, i32, f32]),
        "parc_mopt_kernel_times": (rc, [vp, f32p]),
        # motion generator's training loss
        "parc_mloss_create": (rc, [P(ParcMotionLossParams), P(vp)]),
        "parc_mloss_destroy": (None, [vp]),
        "parc_mloss_eval": (rc, [vp, P(ParcMotionLossArgs), vp]),
        "parc_mloss_kernel_times": (rc, [vp, f32p]),
        # motion-terrain analysis
        "parc_mterr_create": (rc, [P(ParcMotionTerrainParams), P(vp)]),
        "parc_mterr_destroy": (None, [vp]),
        "parc_mterr_set_clips": (rc, [vp, P(ParcMotionOptClips)]),
        "parc_mterr_run": (rc, [vp, f32p, i32p, f32p, P(i64)]),
        "parc_mterr_get_mask_inds": (rc, [vp, i32p]),
        "parc_mterr_get_min_heights": (rc, [vp, f32p, i32p]),
        "parc_mterr_point_sdf": (rc, [vp, i64, i32, f32p, f32p]),
        "parc_mterr_kernel_times": (rc, [vp, f32p]),
        # motion-window sampler
        "parc_msamp_create": (rc, [P(ParcMotionSamplerParams), P(vp)]),
        "parc_msamp_destroy": (None, [vp]),
        "parc_msamp_set_clips": (rc, [vp, P(ParcMotionOptClips), P(ParcMotionSamplerClipInfo)]),
        "parc_msamp_sample_with": (rc, [vp, plan_s, out_s, vp]),
        "parc_msamp_draw_plan": (rc, [vp, u64, plan_s, vp]),
        "parc_msamp_sample": (rc, [vp, u64, plan_s, out_s, vp]),
        "parc_msamp_enumerate": (rc, [vp, i32, out_s, vp]),
        "parc_msamp_plan_status": (rc, [vp, vp, i32p]),
        "parc_msamp_kernel_times": (rc, [vp, f32p]),
        # path planner
        "parc_pathplan_create": (rc, [P(ParcPathPlanParams), P(vp)]),
        "parc_pathplan_destroy": (None, [vp]),
        "parc_pathplan_run": (rc, [vp, i32, f32p, i32p, i32p, u64, u64, P(ParcPathPlanOutputs)]),
        "parc_pathplan_get_graph": (rc, [vp, i32, i32, u8p, u8p, u32p]),
        "parc_pathplan_kernel_times": (rc, [vp, f32p]),
        # terrain generator
        "parc_tgen_create": (rc, [P(ParcTerrainGenParams), P(vp)]),
        "parc_tgen_destroy": (None, [vp]),
        "parc_tgen_draw_plan": (rc, [vp, u64, u64, P(ParcTerrainGenPlan), vp]),
        "parc_tgen_generate_with": (rc, [vp, P(ParcTerrainGenPlan), vp, i32, vp]),
        "parc_tgen_generate": (rc, [vp, i32, u64, u64, vp, vp]),
        "parc_tgen_kernel_times": (rc, [vp, f32p]),
        # motion-terrain augmenter
        "parc_maug_create": (rc, [P(ParcMotionAugParams), P(vp)]),
        "parc_maug_destroy": (None, [vp]),
        "parc_maug_set_clips": (rc, [vp, P(ParcMotionOptClips), P(ParcMotionAugClipInfo)]),
        "parc_maug_draw_plan": (rc, [vp, u64, u64, i32, P(ParcMotionAugPlan), vp]),
        "parc_maug_augment_with": (rc, [vp, P(ParcMotionAugPlan), i32, vp, P(ParcMotionAugSizes)]),
        "parc_maug_augment": (rc, [vp, i32, u64, u64, i32, vp, P(ParcMotionAugSizes)]),
        "parc_maug_get_result": (rc, [vp, P(ParcMotionAugOutputs), vp]),
        "parc_maug_plan_status": (rc, [vp, vp, i32p]),
        "parc_maug_kernel_times": (rc, [vp, f32p]),
        # motion generator
        "parc_mdm_create": (rc, [P(ParcMdmParams), P(vp)]),
        "parc_mdm_destroy": (None, [vp]),
        "parc_mdm_embed_conds": (rc, [vp, P(ParcMdmConds), vp, vp, vp]),
        "parc_mdm_forward": (rc, [vp, vp, i32, i32, vp, vp]),
        "parc_mdm_update": (rc, [vp, i32, vp, vp, f32, vp, i32, f32, f32, f32, vp, vp, vp]),
        "parc_mdm_sample": (rc, [vp, P(ParcMdmConds), P(ParcMdmSampleArgs), vp]),
        "parc_mdm_draw_noise": (rc, [vp, i32, u64, u64, u32, vp, vp]),
        "parc_mdm_kernel_times": (rc, [vp, f32p]),
        "parc_mdm_describe": (rc, [vp, i64p]),
        # path-following motion generation
        "parc_mpath_create": (rc, [P(ParcMdmPathParams), P(vp)]),
        "parc_mpath_destroy": (None, [vp]),
        "parc_mpath_set_scene": (rc, [vp, f32p, i32, i32, i32, f32p, f32, f32, f32p, i32p, i32, i32p, i32]),
        "parc_mpath_conds": (rc, [vp, vp, i32, i32, P(ParcMdmPathCondOut), vp]),
        "parc_mpath_append": (rc, [vp, P(ParcMdmPathAppendArgs), vp]),
        "parc_mpath_rollout": (rc, [vp, P(ParcMdmPathRolloutArgs), vp]),
        "parc_mpath_kernel_times": (rc, [vp, f32p]),
        "parc_mpath_describe": (rc, [vp, i64p]),
        # rollout selection
        "parc_msel_create": (rc, [P(ParcPathSelectParams), P(vp)]),
        "parc_msel_destroy": (None, [vp]),
        "parc_msel_run": (rc, [vp, P(ParcPathSelectArgs), vp]),
        "parc_msel_results": (rc, [vp, P(ParcPathSelectResults), vp]),
        "parc_msel_gather": (rc, [vp, i32p, i32, f32p, i64, vp]),
        "parc_msel_kernel_times": (rc, [vp, f32p]),
        "parc_msel_describe": (rc, [vp, i64p]),
        # hesitation-frame removal
        "parc_medit_create": (rc, [P(ParcMotionEditParams), P(vp)]),
        "parc_medit_destroy": (None, [vp]),
        "parc_medit_set_clips": (rc, [vp, P(ParcMotionOptClips)]),
        "parc_medit_run": (rc, [vp, i32p, i32p, P(i64)]),
        "parc_medit_get_frames": (rc, [vp, f32p, f32p, f32p, f32p]),
        "parc_medit_get_pair_rows": (rc, [vp, i32, u64p]),
        "parc_medit_get_flags": (rc, [vp, u64p, u64p]),
        "parc_medit_kernel_times": (rc, [vp, f32p]),
        # contact labelling
        "parc_mlabel_create": (rc, [P(ParcMotionLabelParams), P(vp)]),
        "parc_mlabel_destroy": (None, [vp]),
        "parc_mlabel_set_clips": (rc, [vp, P(ParcMotionOptClips)]),
        "parc_mlabel_run": (rc, [vp, i32, i32, i32, f32, i32]),
        "parc_mlabel_get_frames": (rc, [vp, f32p, f32p]),
        "parc_mlabel_get_gap": (rc, [vp, f32p]),
        "parc_mlabel_get_lift": (rc, [vp, f32p]),
        "parc_mlabel_get_hand_sd": (rc, [vp, f32p]),
        "parc_mlabel_resample": (rc, [vp, i64p, f32p, f32p, f32p, f32p, f32p, f32p]),
        "parc_mlabel_kernel_times": (rc, [vp, f32p]),
    }


SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(SIGNATURES)
_lib = None


def load():
    """Load the HIP library; raises if it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback for the env step.")
    import torch  # noqa: F401  the process must hold ONE HIP runtime (torch's): load it before the library binds to libamdhip64
    lib = C.CDLL(LIB_PATH)
    stale = f"{LIB_PATH} is a stale build (ABI mismatch): rebuild with `python -c 'import __graft_entry__ as g; g.build()'`"
    if not hasattr(lib, "parc_abi_version") or lib.parc_abi_version() != ABI_VERSION or any(not hasattr(lib, s) for s in EXPORTED_SYMBOLS):
        raise RuntimeError(stale)
    lib.parc_build_flags.restype = C.c_char_p
    flags = lib.parc_build_flags().decode()
    missing = [f for f in REQUIRED_BUILD_FLAGS if f not in flags.split()]
    if any(m in flags for m in TEST_BUILD_MARKERS) and os.environ.get("PARC_ALLOW_TEST_BUILD") != "1":
        raise RuntimeError(f"{LIB_PATH} is a test-only build ('{flags}'): the product never loads it")
    if missing:  # an SLP-vectorised k_dynamics_wave computes wrong inertias; contraction breaks the 1e-5 parity
        raise RuntimeError(f"{LIB_PATH} was built with '{flags}': missing {missing}; rebuild with __graft_entry__.build()")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


# parc_test_quat_op selectors (include/parc_env.h)
QOP = {"mul": 0, "rotate": 1, "conj": 2, "pos": 3, "normalize3": 4, "to_axis_angle": 5, "aa_to_quat": 6, "exp_map_to_quat": 7,
       "to_exp_map": 8, "diff_angle": 9, "normalize": 10, "to_tan_norm": 11, "slerp": 12, "heading": 13, "heading_quat_inv": 14,
       "diff": 15, "rotate_2d": 16, "slerp_rr": 17}
# -pragma-unroll-threshold: without it the unrolled body loops of k_dynamics_wave stay rolled, its per-body register arrays become ~1 KB of
# scratch per lane and the kernel is several times slower -- a library built without it is refused like one built with SLP
REQUIRED_BUILD_FLAGS = ("-fno-slp-vectorize", "-ffp-contract=off", "-pragma-unroll-threshold=1048576")
# defines of TEST-ONLY builds (__graft_entry__.BREAK_FLAGS): load() refuses a library whose build-flag string carries one unless the
# caller opts in (PARC_ALLOW_TEST_BUILD=1, set by the one test that loads the break-flag variant)
TEST_BUILD_MARKERS = ("-DPARC_TEST_BREAK_FLAG",)


class ParcError(RuntimeError):
    pass


def csrc_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources + the C-ABI header: profiles/*.json carry it, so that bench.py attaches
    counter-derived figures only to the build they were collected on."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(_HERE, "csrc")
    for f in sorted(os.listdir(csrc)) + [os.path.join("..", "..", "include", "parc_env.h")]:
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    return h.hexdigest()[:16]


def check(rc):
    if rc != 0:
        raise ParcError(f"libparc_env error {rc}: {load().parc_last_error().decode()}")


def device_index(device) -> int:
    """The ordinal of ``"cuda:N"`` (a string or a ``torch.device``); 0 when none is given."""
    dev = str(device)
    return int(dev.split(":")[1]) if ":" in dev else 0


def destroy_handle(obj, destroy: str):
    """Release ``obj._h`` through ``obj._lib.<destroy>`` and clear it; safe on an object whose constructor did not finish."""
    h = getattr(obj, "_h", None)
    if h is not None and h.value:
        getattr(obj._lib, destroy)(h)
    obj._h = None


def np_f32p(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(f32p)


def np_i32p(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(i32p)


def make_char_model(cm) -> ParcCharModel:
    """Pack a :class:`parc_amd.char_model.CharModel` into the C struct."""
    m = ParcCharModel()
    nb = cm.get_num_bodies()
    if nb > 15:
        raise ValueError("at most 15 bodies are supported by the gfx950 lane map")
    m.num_bodies = nb
    m.dof_size = cm.get_dof_size()
    jt, ax, di = cm.joint_type_array(), cm.joint_axis_array(), cm.dof_idx_array()
    for b in range(nb):
        m.parent[b] = int(cm._parent_indices[b])
        m.joint_type[b] = int(jt[b])
        m.dof_idx[b] = int(di[b])
        for k in range(3):
            m.local_translation[b][k] = float(cm._local_translation[b][k])
            m.joint_axis[b][k] = float(ax[b][k])
        for k in range(4):
            m.local_rotation[b][k] = float(cm._local_rotation[b][k])
    paths = cm.fk_paths(MAX_FK_PATHS, MAX_FK_DEPTH)
    for p in range(MAX_FK_PATHS):
        for d in range(MAX_FK_DEPTH):
            m.fk_paths[p][d] = int(paths[p, d])
    return m
