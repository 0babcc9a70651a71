/*
 * parc_env.h — C-ABI of libparc_env.so: the MI355X (gfx950) motion-tracking environment.
 *
 * This is the drop-in boundary for the reference's per-env step.  The reference has no FFI: the
 * hot path sits behind the Python class contract BaseEnv (PARC/motion_tracker/envs/base_env.py:20-72)
 * as driven by BaseAgent (PARC/motion_tracker/learning/base_agent.py:291-370).  A thin Python shim
 * (parc_amd/envs/hip_parkour_env.py, ctypes) implements that class contract on top of the entry points
 * below; each entry point cites the reference code it replaces (file:line relative to /root/reference).
 *
 * Conventions
 *   - plain C, no torch types: pointers + sizes.  "_host" pointers are copied during the call and may
 *     be freed afterwards; "_dev" pointers are device memory OWNED BY THE CALLER (PyTorch tensors) that
 *     must stay alive while bound; the library never frees them.
 *   - every launch goes to the hipStream_t passed in (void* here so that the header needs no HIP
 *     include); nothing in step/reset synchronises with the host.
 *   - return 0 on success, negative ParcStatus on error; parc_last_error() gives a thread-local text.
 *   - single caller thread per handle; handles are independent (one process per GPU needs no locks).
 *   - quaternions are (x, y, z, w); all floating point is fp32; row-major [N][...] arrays.
 */
#ifndef PARC_ENV_H
#define PARC_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_ABI_VERSION 6
#define PARC_MAX_BODIES 16   /* 15 quats + root position share one 16-lane group */
#define PARC_MAX_DOFS 40     /* dof velocities live in floats [88,128) of a 128-float frame record */
#define PARC_MAX_TAR_STEPS 6 /* 2 + steps skeletons <= 8 lane groups of 8 */
#define PARC_MAX_KEY_BODIES 8
#define PARC_MAX_FK_PATHS 8
#define PARC_MAX_FK_DEPTH 8
#define PARC_MAX_GEOMS 24

typedef enum {
    PARC_OK = 0,
    PARC_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    PARC_ERR_HIP = -2,         /* a HIP runtime call failed */
    PARC_ERR_STATE = -3,       /* call order (e.g. step before bind/load) */
    PARC_ERR_NO_DEVICE = -4    /* no gfx950 device visible */
} ParcStatus;

typedef enum { PARC_JOINT_ROOT = 0, PARC_JOINT_HINGE = 1, PARC_JOINT_SPHERICAL = 2, PARC_JOINT_FIXED = 3 } ParcJointType;
typedef enum { PARC_DONE_NULL = 0, PARC_DONE_FAIL = 1, PARC_DONE_SUCC = 2, PARC_DONE_TIME = 3 } ParcDoneFlag; /* base_env.py:14-18 */
typedef enum { PARC_LOOP_CLAMP = 0, PARC_LOOP_WRAP = 1 } ParcLoopMode;                                        /* motion_lib.py:14-16 */
typedef enum { PARC_GEOM_BOX = 0, PARC_GEOM_SPHERE = 1, PARC_GEOM_CAPSULE = 2 } ParcGeomType;

typedef struct ParcEnv ParcEnv;

/* Character tables — what KinCharModel.load_char_file / init produce (kin_char_model.py:154-190,235). */
typedef struct {
    int32_t num_bodies;                                  /* B, body 0 = root */
    int32_t dof_size;                                    /* D */
    int32_t parent[PARC_MAX_BODIES];
    float local_translation[PARC_MAX_BODIES][3];
    float local_rotation[PARC_MAX_BODIES][4];
    int32_t joint_type[PARC_MAX_BODIES];                 /* ParcJointType */
    float joint_axis[PARC_MAX_BODIES][3];
    int32_t dof_idx[PARC_MAX_BODIES];
    int32_t fk_paths[PARC_MAX_FK_PATHS][PARC_MAX_FK_DEPTH]; /* root-to-leaf body chains, -1 padded */
} ParcCharModel;

/* Rigid-body / actuator parameters the reference hands to Isaac Gym through the MJCF
 * (ig_char_env.py:100-143, humanoid.xml) and the sim block of dm_env_default.yaml:175-186. */
/* ControlMode of the reference (ig_char_env.py:21-26).  pd: the action is the PD position target (exp-map per spherical joint), clipped to the action
 * bounds (implicit drive, PhysX DOF_MODE_POS).  vel: velocity target, drive force = damping * (action - dof_vel) (DOF_MODE_VEL, stiffness 0).  torque: the
 * clipped action is the joint torque (DOF_MODE_EFFORT).  pd_exp / pd_1d: the explicit PD torque of ig_char_env.py:399-421, target = the action as given
 * (not clipped, :500-503), limited to the motor efforts; pd_1d needs a character whose joints all have one dof (the reference asserts it, :246-250).
 * This library forms that torque once per control step, from the state at its start, and holds it; the reference forms it again at every sim step
 * (_step_sim -> _apply_forces, :369-397).  A known deviation: ADVICE.md item 1; the one place that decides it is joint_control_* in parc_dynamics.hpp. */
#define PARC_CTRL_PD 0
#define PARC_CTRL_VEL 1
#define PARC_CTRL_TORQUE 2
#define PARC_CTRL_PD_EXP 3
#define PARC_CTRL_PD_1D 4
typedef struct {
    int32_t num_geoms;
    int32_t geom_body[PARC_MAX_GEOMS];
    int32_t geom_type[PARC_MAX_GEOMS];
    float geom_pos[PARC_MAX_GEOMS][3];   /* sphere/box centre, capsule end 0 (body frame) */
    float geom_pos2[PARC_MAX_GEOMS][3];  /* capsule end 1 */
    float geom_size[PARC_MAX_GEOMS][3];  /* sphere r | box half extents | capsule r */
    float geom_density[PARC_MAX_GEOMS];
    float dof_stiffness[PARC_MAX_DOFS];  /* PD kp (MJCF joint stiffness) */
    float dof_damping[PARC_MAX_DOFS];    /* PD kd */
    float dof_armature[PARC_MAX_DOFS];
    float dof_effort[PARC_MAX_DOFS];     /* motor gear = max torque */
    float dof_lower[PARC_MAX_DOFS];
    float dof_upper[PARC_MAX_DOFS];
    float gravity_z;                     /* ig_env.py:142-145 */
    float sim_dt;                        /* 1 / sim_freq */
    int32_t sim_steps;                   /* sim_freq / control_freq (ig_env.py:113) */
    int32_t substeps;                    /* dm_env_default.yaml:186 */
    int32_t solver_iterations;           /* num_position_iterations */
    float friction;                      /* ig_util.py:10 */
    float restitution;
    float contact_offset;
    float max_depenetration_velocity;
    float angular_damping;               /* ig_char_env.py:142 */
    float max_angular_velocity;          /* ig_char_env.py:143 */
    int32_t control_mode;                /* env.control_mode (ig_char_env.py:21-26,95): PARC_CTRL_*; what `action` means (ig_char_env.py:488-506) */
} ParcDynamicsParams;

/* Environment constants — the keys IGParkourEnv.__init__ reads (ig_parkour_env.py:43-149). */
typedef struct {
    uint32_t abi_version;       /* PARC_ABI_VERSION */
    uint32_t struct_size;       /* sizeof(ParcEnvConfig) */
    int32_t device;             /* HIP device ordinal */
    int32_t num_envs;           /* N local envs of this handle */
    ParcCharModel model;
    int32_t num_key_bodies;
    int32_t key_body_ids[PARC_MAX_KEY_BODIES];
    int32_t num_tar_obs_steps;
    int32_t tar_obs_steps[PARC_MAX_TAR_STEPS];
    int32_t num_rays;
    const float *ray_points_host;            /* [R][2] geom_util.get_xy_points_cone:251 */
    double control_dt;                       /* 1 / control_freq (python double, cast like torch does) */
    float episode_length;
    float min_obs_h, max_obs_h;
    float pose_w, vel_w, root_pos_w, root_vel_w, key_pos_w;   /* already divided by their sum (:91-101) */
    float joint_err_w[PARC_MAX_BODIES];      /* [J] */
    float dof_err_w[PARC_MAX_DOFS];          /* [D] */
    float contact_weights[PARC_MAX_BODIES];  /* [B] */
    float pose_termination_dist[PARC_MAX_BODIES]; /* [J] */
    float root_pos_termination_dist, root_rot_termination_angle;
    int32_t enable_early_termination, pose_termination, track_root, track_root_h;
    int32_t report_tracking_error;
    float fail_rate_ema_weight;              /* dm_env.py:88 */
    float min_motion_weight;                 /* dm_env.py:26 */
    float rand_root_pos_offset_scale;        /* mgdm_dm_util.py:102-106 */
    int32_t rand_reset;                      /* dm_env.py:500-504 */
    int32_t demo_mode;                       /* dm_env.py:479-480 */
    const float *env_offsets_host;           /* [N][3] ig_parkour_env.py:389-398 (global env ids of this shard) */
    float action_low[PARC_MAX_DOFS], action_high[PARC_MAX_DOFS]; /* ig_char_env.py:307-347 */
    int32_t body_pos_from_fk;                /* 1: rigid-body positions := FK(char state) inside the step
                                                (reduced-coordinate sim / kinematic mode); 0: read bound buffer */
    int32_t enable_dynamics;                 /* 0 = kinematic-only step (state injected by the caller) */
    ParcDynamicsParams dynamics;             /* used when enable_dynamics */
    uint64_t seed;
    /* `contact_bodies` (ig_parkour_env.py:62, dm_env_default.yaml:8; [] by default): bit b set = body b may touch the ground.  Non-zero
     * switches on the fall rule of compute_done (mgdm_dm_util.py:349-360): FAIL when some OTHER body carries a contact-force component
     * above 0.1 and some other body is lower than termination_height above the terrain under it (RefCharEnv.update_done :147-152). */
    uint32_t contact_body_mask;
    float termination_height;                /* ig_parkour_env.py:63 */
    /* `global_obs` (ig_parkour_env.py:83; false by default): compute_char_obs (ig_char_env.py:586-589, :603) and compute_tar_obs
     * (mgdm_dm_util.py:417) leave root rotation, root velocities, root / key offsets in the global frame. */
    int32_t global_obs;
    /* `global_root_height_obs` (ig_parkour_env.py:84, passed on as compute_char_obs's root_height_obs, :904; false by default): the root
     * height is one more observation in FRONT of the character block (ig_char_env.py:620-622): every later offset moves by one. */
    int32_t global_root_height_obs;
    /* `use_contact_info` (ig_parkour_env.py:72-73; true by default): false drops the target / character contact blocks of the observation
     * (:927-946) and the contact term of the reward (:1032-1040).  `enable_tar_obs` (:83; true by default): false drops the look-ahead
     * target block (mgdm_dm_util.py:482-493) and, with it, the target contact block (:928-930). */
    int32_t use_contact_info, enable_tar_obs;
    /* Developer / test switches, "key=value;key=value" (NULL or "" = none; the product never sets any).  They are part of the configuration
     * so that a measurement can state them (parc_env_describe): the library reads no environment variable.
     *   segments=none|capsules   drop the collision segments (all / the sole edges of boxes)      dtang=<float>   tangential contact damping
     *   kernel=coop|thread       force one of the general dynamics kernels                         man_period=<n>  contact discovery every n substeps
     *   no_residual=1            no root-position residual (precision test)                        ema_leader=1 | curriculum_two_launches=1
     *                                                                                              force one of the curriculum launch paths */
    const char *dev_options;
} ParcEnvConfig;

/* Motion clips as MotionLib._load_motion_file receives them (motion_lib.py:255-401); the library
 * derives root_vel / root_ang_vel / dof_vel on the device and packs 512-byte frame records. */
typedef struct {
    int32_t num_motions;
    const int32_t *num_frames_host;   /* [M] */
    const int32_t *fps_host;          /* [M] */
    const int32_t *loop_modes_host;   /* [M] ParcLoopMode */
    const double *weights_host;       /* [M] un-normalised */
    const float *root_pos_host;       /* [F][3], clips concatenated */
    const float *root_rot_host;       /* [F][4] */
    const float *joint_rot_host;      /* [F][J][4] */
    const float *contacts_host;       /* [F][B] or NULL (=> zeros, motion_lib.py:345-347) */
} ParcMotionClips;

/* Device buffers owned by the caller.  NULL = that optional output is not written. */
typedef struct {
    /* simulator-side character state (ig_char_env.py:173-196): read by step, written by reset/dynamics */
    float *char_root_pos, *char_root_rot, *char_root_vel, *char_root_ang_vel; /* [N][3|4|3|3] */
    float *char_dof_pos, *char_dof_vel;                                       /* [N][D] */
    float *char_body_pos;                                                     /* [N][B][3] */
    float *contact_forces;                                                    /* [N][B][3] */
    /* bookkeeping (dm_env.py:76-78, ig_parkour_env.py:616-621) */
    int32_t *motion_ids, *terrain_ids;                                        /* [N] */
    float *time_offsets;                                                      /* [N] */
    int32_t *timestep;                                                        /* [N] */
    float *time;                                                              /* [N] optional */
    int64_t *ep_num;                                                          /* [N] optional */
    /* outputs of the step (BaseEnv.step contract) */
    float *obs;                                                               /* [N][obs_dim] */
    float *reward;                                                            /* [N] */
    int32_t *done;                                                            /* [N] ParcDoneFlag */
    float *reward_terms;                                                      /* [7][N] pose,vel,root_pos,root_vel,key_pos,contact,total */
    float *tracking_error;                                                    /* [N][7] optional */
    /* optional mirrors of the reference's ref_* tensors (ig_parkour_env.py:560-571) */
    float *ref_root_pos, *ref_root_rot, *ref_root_vel, *ref_root_ang_vel;
    float *ref_joint_rot, *ref_dof_pos, *ref_dof_vel, *ref_body_pos, *ref_contacts;
    float *ray_hfs;                                                           /* [N][R] optional */
} ParcEnvBuffers;

const char *parc_last_error(void);
int parc_abi_version(void);

/* IGParkourEnv.__init__ (ig_parkour_env.py:43-149) minus Isaac Gym.  The arguments are checked before the device is touched; on any
 * failure nothing is left allocated and *out is not written.  parc_env_destroy(NULL) is a no-op. */
int parc_env_create(const ParcEnvConfig *cfg, ParcEnv **out);
void parc_env_destroy(ParcEnv *env);
/* obs width for this configuration (IGEnv.get_obs_space, ig_env.py:86-96) */
int parc_env_obs_dim(const ParcEnv *env);

/* MotionLib._load_motion_file (motion_lib.py:255-401).  May be called again: the new set replaces the old one as the last step of the
 * call, and every fail rate starts at 1 (dm_env.py:87).  A call that returns non-zero (PARC_ERR_INVALID: a clip of fewer than 2 frames,
 * fps <= 0, a negative weight, more than 2^30 frames; PARC_ERR_HIP) leaves the handle as it was in every observable way: motion info,
 * fail rates, and what step / reset / the graph step compute.  A successful load whose num_motions differs from the loaded terrain's M
 * drops that terrain (its motion_offsets have one row per motion of the old set): the step-family calls return PARC_ERR_STATE until
 * parc_env_load_terrain is called again.  A reload with the same num_motions keeps the terrain. */
int parc_env_load_motions(ParcEnv *env, const ParcMotionClips *clips);
/* DeepMimicEnv.build_terrain_square / load_terrain result (dm_env.py:157-316,447-463):
 * hf [X][Y] x-major, motion_offsets [M][T][2].  After parc_env_load_motions, with M = its num_motions (else PARC_ERR_STATE).  May be
 * called again; like parc_env_load_motions, a call that returns non-zero leaves the handle, its previous terrain included, as it was. */
int parc_env_load_terrain(ParcEnv *env, const float *hf_host, int32_t X, int32_t Y, float min_x, float min_y,
                          float dx, float dy, const float *motion_offsets_host, int32_t M, int32_t T);
/* IGCharEnv._build_sim_tensors / IGParkourEnv._build_data_buffers tensor views */
int parc_env_bind_buffers(ParcEnv *env, const ParcEnvBuffers *bufs);
/* The state view (SURVEY 8(b) "get_state / set_state"): the character, reference and bookkeeping state lives in the
 * caller's device buffers bound above; this returns those pointers, reading them is get_state, writing them before
 * parc_env_step is set_state (that is how the kinematic configuration injects the character state). */
int parc_env_get_buffers(ParcEnv *env, ParcEnvBuffers *out);

/* IGEnv.step (ig_env.py:66-84): clip action -> [dynamics] -> _post_physics_step.  action_dev [N][D]
 * may be NULL when enable_dynamics == 0. */
int parc_env_step(ParcEnv *env, const float *action_dev, void *stream);
/* IGParkourEnv.reset (ig_parkour_env.py:809-829) with device RNG.  env_ids_dev int64 [k]; k < 0 = all. */
int parc_env_reset(ParcEnv *env, const int64_t *env_ids_dev, int32_t k, void *stream);
/* Same with the random draws injected (parity tests): all arrays device, length k. */
int parc_env_reset_with(ParcEnv *env, const int64_t *env_ids_dev, int32_t k, const int32_t *motion_ids_dev,
                        const int32_t *terrain_ids_dev, const float *t0_dev, const float *xy_noise_dev, void *stream);
/* BaseAgent._reset_done_envs (base_agent.py:366-370) fused on the device: resets every env whose done flag was
 * raised by the last parc_env_step, using the step's own compacted done list (no nonzero(), no host sync). */
int parc_env_reset_done(ParcEnv *env, void *stream);
/* _update_observations(env_ids) (ig_env.py:396-403): rays + obs rows only. k < 0 = all. */
int parc_env_compute_obs(ParcEnv *env, const int64_t *env_ids_dev, int32_t k, void *stream);

/* dm_env.py:84-88 curriculum state */
int parc_env_get_fail_rates(ParcEnv *env, float *out_host, int32_t M);
int parc_env_set_fail_rates(ParcEnv *env, const float *in_host, int32_t M);
/* per-motion tables derived at load (motion_lib.py:361-384); any pointer may be NULL */
int parc_env_get_motion_info(ParcEnv *env, float *lengths_host, float *weights_host, int32_t M);
/* `never_done` (ig_parkour_env.py:59,980): done flags read NULL after update_done, so the agent resets nothing and
 * parc_env_reset_done resets nobody; the fail-rate curriculum still sees the episode ends, as in the reference. */
int parc_env_set_never_done(ParcEnv *env, int32_t never_done);
/* reset sampling switches of DeepMimicEnv: `rand_reset` / `demo_mode` (dm_env.py:28-29,479-505; set_demo_mode :737-741) and the scale of the random
 * root offset; the per-env start time as a fraction of the clip length used when rand_reset is off (set_motion_start_time_fraction, dm_env.py:743-744,
 * read at :502; the record mode's retry schedule sets it) */
int parc_env_set_rand_reset(ParcEnv *env, int32_t rand_reset, int32_t demo_mode, float root_pos_offset_scale);
int parc_env_set_start_time_fraction(ParcEnv *env, const float *frac_dev /* [N] or NULL */);

/* Stand-alone operators on device arrays (cfg-1 plumbing and the KinCharModel / MotionLib mirrors):
 * kin_char_model.py:586,601,617; motion_lib.py:94 */
int parc_dof_to_rot(ParcEnv *env, const float *dof_dev, float *joint_rot_dev, int32_t n, void *stream);
int parc_rot_to_dof(ParcEnv *env, const float *joint_rot_dev, float *dof_dev, int32_t n, void *stream);
int parc_forward_kinematics(ParcEnv *env, const float *root_pos_dev, const float *root_rot_dev,
                            const float *joint_rot_dev, float *body_pos_dev, float *body_rot_dev, int32_t n, void *stream);
int parc_calc_motion_frame(ParcEnv *env, const int32_t *motion_ids_dev, const float *times_dev, int32_t n,
                           float *root_pos_dev, float *root_rot_dev, float *root_vel_dev, float *root_ang_vel_dev,
                           float *joint_rot_dev, float *dof_vel_dev, float *contacts_dev, void *stream);
/* TEST ENTRY POINT: one of the quaternion device functions of parc_math.hpp (the restatements of torch_util.py:6-530 that
 * the kernels inline) applied element-wise to device arrays, so that the reference's edge-case vectors (w < 0, tiny angles,
 * |sin| < 1e-3, |cos| >= 1, exp maps beyond pi; tests/golden/quat_ops.npz) reach the DEVICE code and not only the CPU oracle.
 * a: [n][4] (ops on quaternions) or [n][3] (PARC_QOP_NORMALIZE3 / EXP_MAP_TO_QUAT / AA_TO_QUAT axis / ROTATE_2D vector in
 * the first two components); b: second operand ([n][4], or [n][3] for QUAT_ROTATE) or NULL; t: [n] scalar (slerp
 * parameter / angle) or NULL; out: [n][PARC_QOP out width: 4, 3, 6 (tan-norm), 1 or 2]. */
enum {
    PARC_QOP_MUL = 0, PARC_QOP_ROTATE = 1, PARC_QOP_CONJ = 2, PARC_QOP_POS = 3, PARC_QOP_NORMALIZE3 = 4, PARC_QOP_TO_AXIS_ANGLE = 5 /* out [n][4]: axis, angle */,
    PARC_QOP_AA_TO_QUAT = 6, PARC_QOP_EXP_MAP_TO_QUAT = 7, PARC_QOP_TO_EXP_MAP = 8, PARC_QOP_DIFF_ANGLE = 9, PARC_QOP_NORMALIZE = 10,
    PARC_QOP_TO_TAN_NORM = 11, PARC_QOP_SLERP = 12, PARC_QOP_HEADING = 13, PARC_QOP_HEADING_QUAT_INV = 14, PARC_QOP_DIFF = 15,
    PARC_QOP_ROTATE_2D = 16, PARC_QOP_SLERP_RR = 17 /* slerp as k_env_post evaluates it: reduced-range sin / acos polynomials, DESIGN.md 4 */
};
int parc_test_quat_op(int32_t op, const float *a_dev, const float *b_dev, const float *t_dev, int32_t n, float *out_dev, void *stream);

/* The compiler flags the library was built with (set by the build recipe): the loader refuses a library whose flags lack
 * -fno-slp-vectorize / -ffp-contract=off (toolchain note). */
const char *parc_build_flags(void);

/* copy the derived frame tables back (tests): [F][3],[F][3],[F][D] */
int parc_env_get_frame_vel_tables(ParcEnv *env, float *root_vel_host, float *root_ang_vel_host, float *dof_vel_host);

/* Timing of the dominant kernel with hipEvents on the launch stream (bench.py roofline leg). */
int parc_env_profile_step(ParcEnv *env, const float *action_dev, void *stream, int32_t iters, float *avg_ms_out,
                          float *avg_post_kernel_ms_out);

/* The waves of a k_dynamics_wave block hand records to each other through LDS flags; a wait is bounded so that a protocol
 * error cannot hang the GPU.  Number of waits that ever hit the bound on this device (synchronises; must be 0; < 0 = error). */
/* What this handle resolved to, "key=value;..." (dynamics kernel, envs per block, collision points / segments, contact parameters, manifold
 * period and margins, curriculum path, the dev_options it was created with): bench.py records it with every measurement.  The string
 * lives as long as the handle. */
const char *parc_env_describe(ParcEnv *env);

int parc_env_dynamics_timeouts(ParcEnv *env);
/* The same two counters {flag-wait timeouts, manifold drops} as two words of host-mapped pinned memory that the first launch after every
 * step refreshes: readable WITHOUT a synchronisation (stale by at most one step).  NULL when pinned memory could not be mapped. */
const unsigned int *parc_env_health_words(ParcEnv *env);
/* Contact planes the dynamics kernel had no room for since the library was loaded (its per-lane plane list and overflow area were full):
 * must stay 0.  Synchronises the device. */
int parc_env_dynamics_manifold_drops(ParcEnv *env);

/* average duration of k_dynamics in the last parc_env_profile_step call (0 when dynamics is off) */
float parc_env_last_dynamics_ms(ParcEnv *env);

/* `env._episode_length = x` (dm_motion_recorder.py:55 raises it to 1000 s so that only the clip end finishes an episode) */
int parc_env_set_episode_length(ParcEnv *env, float seconds);

/* One control step INCLUDING the reset of the envs it finished (== parc_env_step + parc_env_reset_done) as a single
 * hipGraph launch: the ~10 dependent kernel launches are captured once and replayed, which removes the host-side launch
 * cost that dominates below ~10 000 envs.  The action is read from the buffer bound with parc_env_bind_action (write the
 * policy output there); the graph is re-captured automatically when a setter changes something it bakes in.  Kernel
 * timing events and the recorder are not part of the graph: use parc_env_step for those. */
int parc_env_bind_action(ParcEnv *env, const float *action_dev);
int parc_env_step_reset_graph(ParcEnv *env, void *stream);

/* TD(lambda) returns of a rollout (rl_util.py:7-30; called from ppo_agent._build_train_data): one thread per env walks the
 * T steps backwards,  ret[T-1] = r + g*nv,  ret[i] = r[i] + g*((1 - l_i)*nv[i] + l_i*ret[i+1]),  l_i = lambda*(1 - [done[i] != 0]).
 * All arrays are device pointers laid out [T][N] (the experience buffer's layout); same fp32 operation order as the
 * reference's Python loop, so results are bit-identical to it.  Needs no env handle. */
int parc_td_lambda_return(const float *reward, const float *next_vals, const int32_t *done, float discount, float td_lambda,
                          int32_t T, int32_t N, float *ret_out, void *stream);

/* Observation normalisation fused with the experience-buffer write (normalizer.py:87-90 +
 * experience_buffer.record): one pass reads x [n][dim] and writes  norm = clamp((x - mean) / std, -clip, clip)  and, when
 * copy_out is not NULL, the unmodified row into the rollout buffer slot.  Same fp32 operations in the same order as the
 * three torch kernels it replaces (IEEE division), so `norm` is bit-identical to Normalizer.normalize. */
int parc_normalize_record(const float *x, const float *mean, const float *std, float clip, float *norm_out, float *copy_out,
                          int64_t n, int32_t dim, void *stream);

/* Minibatch gather of the experience buffer (experience_buffer.py:81-89: `{k: v[idx] for k, v in flat_buffers}`, one indexing kernel per
 * buffer in the reference).  ONE launch copies, for every sampled row r < n, row (idx[r] mod count) of each of the
 * num_buffers flat buffers into row r of its contiguous minibatch tensor: src[b] / dst[b] are device pointers, row_bytes[b] the size of one
 * row of buffer b in bytes (any element type: the copy is byte-exact, i.e. bit-identical to index_select).  idx: device int64.  Rows of
 * at least 64 bytes are moved by a wavefront each (16-byte lanes where the row is 16-byte aligned), narrower ones by one thread per row. */
#define PARC_MAX_GATHER_BUFFERS 16
int parc_gather_rows(int32_t num_buffers, const void *const *src_dev, void *const *dst_dev, const int64_t *row_bytes, const int64_t *idx_dev,
                     int64_t n, int64_t count, void *stream);

/* Recorder (IGParkourEnv.write_agent_states, ig_parkour_env.py:759-796; driven by dm_motion_recorder.py:52-121).
 * The reference appends one row per recording env to Python lists every step; here the rows go to device ring buffers
 * owned by the caller:
 *   frames  [cap][N][PARC_REC_WIDTH] f32: root_pos 3 (env-local) | root_rot 4 (xyzw) | joint_rot (B-1) x 4 | contacts B
 *           (contact = |F_b| > 1e-5, _get_char_state ig_parkour_env.py:664-685; the reference stores exp maps / dofs and
 *           converts on save, the motion-terrain file format holds quaternions: file_io.py:8-16)
 *   obs     [cap][N][obs_dim] f32 or NULL (record_obs)
 *   count   [N] i32 rows written; writing [N] u8 (1 = this env is recording); n_writing [1] i32 number of such envs
 * parc_env_record_frame appends the CURRENT state of every recording env (call it after reset for frame 0 and after
 * every step, as the reference does) and ends the recording of envs whose done flag is FAIL; record_ref != 0 stores the
 * reference-motion state instead of the character's (needs the ref_* mirrors of ParcEnvBuffers). */
#define PARC_REC_WIDTH(B) (3 + 4 + 4 * ((B) - 1) + (B))
int parc_env_record_bind(ParcEnv *env, float *frames_dev, float *obs_dev, int32_t cap, int32_t *count_dev, uint8_t *writing_dev,
                         int32_t *n_writing_dev, int32_t record_ref);
int parc_env_record_frame(ParcEnv *env, void *stream);

/* Kernel timing over a run of ordinary parc_env_step calls (what bench.py reports as the roofline's kernel duration).
 * While enabled, every step records three events on the caller's stream (before the dynamics kernel, after it, after
 * the observation kernels); nothing synchronises.  parc_env_get_kernel_timing waits for the last step, returns the
 * average duration of the dynamics kernel and of the observation kernels (k_env_post<STEP>, preceded by k_env_prep when
 * the dynamics kernel did not write the prep records itself) over the steps since the last call, and
 * clears the record. */
int parc_env_set_kernel_timing(ParcEnv *env, int32_t enable);
int parc_env_get_kernel_timing(ParcEnv *env, double *dynamics_ms_avg, double *obs_ms_avg, int32_t *steps);
/* Per-step samples of the same events (call before parc_env_get_kernel_timing, which clears them): dynamics kernel, observation kernel and
 * the curriculum launches of up to `cap` recorded steps; *steps = steps recorded. */
int parc_env_get_kernel_timing_samples(ParcEnv *env, float *dynamics_ms, float *obs_ms, float *curriculum_ms, int32_t cap, int32_t *steps);

/* name of the dynamics kernel this handle launches ("k_dynamics_wave", "k_dynamics_coop", "k_dynamics"; "" when
 * dynamics is off).  The choice follows the shape of the kinematic tree (see parc_env_create). */
const char *parc_env_dynamics_kernel(ParcEnv *env);

/* instantiation of the observation kernel the bound buffers select: "k_env_post<MODE,true>" when any optional output (the
 * ref_* mirrors, ray_hfs, tracking_error) is bound, "k_env_post<MODE,false>" otherwise (the training / bench configuration);
 * "" before parc_env_bind_buffers.  The parity tests assert which one they exercised. */
const char *parc_env_post_kernel(ParcEnv *env);

/* Headless renderer (the reference's viewer, ig_parkour_env.py:417-441 / :1046-1064 / :1123-1132, without a display): ray-casts the scene of k
 * envs into W x H images on the device.  Scene = what the physics collides with: the heightfield as blocky cell columns (cell (i, j) solid
 * below hf[i][j] over min + (i, j) d +- d/2, walls between neighbours, nothing outside the grid), the simulated character's collision geoms at
 * FK of char_root_pos / rot + char_dof_pos and, with draw_ref, the reference character's at FK of ref_root_pos / rot + ref_joint_rot +
 * ref_offset in (0.5, 0.9, 0.1).  Lambert shading from one sun + ambient, a checker on the column tops, optional hard shadows.
 * Camera: PARC_CAMERA_TRACK looks at the env's root from root + offset; PARC_CAMERA_STILL from eye to target, both relative to the env's origin.
 * The struct carries its own size (checked like ParcEnvConfig's); the ABI version does not change with it.
 * Outputs (caller-owned device buffers, NULL = not written), row-major [k][H][W]:
 *   rgba  u8 x 4;   depth f32 ray distance, +inf for sky;
 *   id    u8: 0 sky, 1 terrain top, 2 terrain wall, 16 + b simulated body b, 32 + b reference body b; bit 0x80 = the point is in shadow.
 * env_ids_dev: int64 [k] device, or NULL for envs 0 .. k-1.  Needs the ref_* mirrors bound when draw_ref is set (else PARC_ERR_STATE). */
#define PARC_CAMERA_TRACK 0
#define PARC_CAMERA_STILL 1
typedef struct {
    uint32_t struct_size;       /* sizeof(ParcRenderParams) */
    int32_t width, height;      /* [8, 4096] */
    int32_t camera_mode;        /* PARC_CAMERA_* */
    float offset[3];            /* TRACK: eye = root + offset (the reference's default camera sits at (0, -5) and 3 m absolute height) */
    float eye[3], target[3];    /* STILL: relative to the env's origin */
    float fov_y;                /* vertical field of view, radians */
    float sun_dir[3];           /* direction toward the sun (normalised by the library) */
    float ref_offset[3];        /* ref_char_offset (ig_parkour_env.py:1131) */
    int32_t draw_ref, shadows, debug_visuals;
} ParcRenderParams;
int parc_env_render(ParcEnv *env, const ParcRenderParams *p, const int64_t *env_ids_dev, int32_t k, uint8_t *rgba_dev, float *depth_dev,
                    uint8_t *id_dev, void *stream);

/* Scene render (the reference's viewer draws every env, ig_parkour_env.py:409-441): ONE W x H image of the terrain and the characters of n
 * envs, each at its state + env_offsets in the one world (envs that track the same clip overlap).  The camera is p's, relative to
 * camera_env exactly as parc_env_render places it for that env (TRACK: eye = its root + offset; STILL: eye and target relative to its
 * origin).  With draw_ref every listed env's reference character is drawn too (+ ref_offset).  Every drawn character casts shadows, also
 * one outside the view; debug_visuals tints the camera env's characters only (the reference tints _camera_env_id, :1046-1064).
 * env_ids_dev: int64 [n] device, or NULL for envs 0 .. n-1; ids outside [0, num_envs) are skipped on the device, characters whose root is
 * not finite are not drawn.  Outputs (caller-owned device buffers, NULL = not written), row-major [H][W]: rgba, depth and id encoded as
 * for parc_env_render; env_map int32 = env of the character hit, -1 for terrain and sky.  Equal distances go to the smaller env, then
 * to the simulated character: two calls on the same state give identical bytes.  Errors: PARC_ERR_INVALID for struct_size, sizes,
 * camera, camera_env outside [0, num_envs) or n outside [1, num_envs]; PARC_ERR_STATE when draw_ref is set without the ref_* mirrors.
 * Device workspace, allocated on the first call (again when n grows) and freed by parc_env_destroy: 2 x (4 x round_up(7 B, 4) + 36)
 * bytes per env of n (B = bodies; 936 B for the 15-body humanoid) + 48 KB of bins.  Everything is enqueued on `stream` (no host sync). */
int parc_env_render_scene(ParcEnv *env, const ParcRenderParams *p, int32_t camera_env, const int64_t *env_ids_dev, int32_t n,
                          uint8_t *rgba_dev, float *depth_dev, uint8_t *id_dev, int32_t *env_map_dev, void *stream);

/* Kinematic motion optimiser (the reference's motion_optimization.py: motion_contact_optimization with the loss
 * motion_terrain_contact_loss_localized, :426-656, and compute_approx_body_constraints' point refinement, :124-146) for B clips at once.
 * Its own handle: nothing is shared with a ParcEnv.  Per frame the parameters are root_pos[3] | root exp map[3] | joint dofs[dof_size]
 * (PARC_MOPT_NP(dof_size) floats); every array below is row-major over the clips' frames concatenated in clip order.
 * Every iteration is one host-driven sequence of short launches; results are deterministic and do not depend on
 * which other clips are in the batch.  Terms follow the reference's LossType order: root pos, root rot, joint rot, smoothness,
 * penetration, contact, sliding, body constraints, jerk. */
#define PARC_MOPT_NUM_TERMS 9
#define PARC_MOPT_MAX_POINTS 512
#define PARC_MOPT_NP(D) (6 + (D))
typedef struct ParcMotionOpt ParcMotionOpt;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionOptParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t num_points;                      /* sample points per frame, [1, PARC_MOPT_MAX_POINTS]; contiguous per body, bodies in order */
    const float *points_host;                /* [num_points][3] body-local */
    const int32_t *point_body_host;          /* [num_points] */
    int32_t geom0_type[PARC_MAX_BODIES];     /* first geom of each body (the body-constraint shape): 0 box, 1 sphere, 2 capsule, -1 none */
    float geom0_offset[PARC_MAX_BODIES][3];
    float geom0_radius[PARC_MAX_BODIES];     /* sphere: radius; box: 1.25 |half extents| (motion_optimization.py:589-602) */
    int32_t contact_body_id[PARC_MAX_BODIES];/* column of the contacts array of each body, -1 when it is not a contact body */
    float weights[PARC_MOPT_NUM_TERMS];      /* w_root_pos .. w_jerk; w_contact = 0 / w_sliding = 0 switch the term off (reported as 0) */
    float max_jerk;                          /* scaled by (1/30)^3 on the device, as the reference does */
    float step_size;                         /* Adam learning rate; betas 0.9 / 0.999, eps 1e-8 (torch.optim.Adam defaults) */
} ParcMotionOptParams;
typedef struct {
    int32_t num_clips;
    const int64_t *frame_off_host;           /* [num_clips + 1] */
    const int64_t *hf_off_host;              /* [num_clips + 1] offsets into hf_host */
    const int64_t *cons_off_host;            /* [num_clips + 1] offsets into the constraint arrays */
    const int32_t *hf_dims_host;             /* [num_clips][2] */
    const float *hf_geom_host;               /* [num_clips][4] min_x, min_y, dx, dy */
    const float *hf_host;                    /* cells, x-major per clip */
    const float *root_pos_host, *root_rot_host, *joint_rot_host, *contacts_host; /* [F][3], [F][4] xyzw, [F][B-1][4], [F][B] */
    const int32_t *cons_body_host;           /* [C] */
    const int32_t *cons_range_host;          /* [C][2] first / last frame */
    const float *cons_point_host;            /* [C][3] */
} ParcMotionOptClips;
int parc_mopt_create(const ParcMotionOptParams *p, ParcMotionOpt **out);
void parc_mopt_destroy(ParcMotionOpt *h);
/* Uploads the clips and sets the iterate to the source (root exp map = quat_to_exp_map, dofs = rot_to_dof); resets Adam.
 * The batch is validated first: PARC_ERR_INVALID leaves the batch loaded before in place and usable.  A valid batch replaces it: the
 * old one is released before the new one is allocated (the handle never holds two), so a failed allocation or upload (PARC_ERR_HIP)
 * leaves the handle without a batch, and every call that needs one returns PARC_ERR_STATE until a parc_mopt_set_clips succeeds. */
int parc_mopt_set_clips(ParcMotionOpt *h, const ParcMotionOptClips *c);
/* Replaces the constraint points (same count as set_clips gave), e.g. after parc_mopt_build_constraints. */
int parc_mopt_set_constraint_points(ParcMotionOpt *h, const float *cons_point_host);
int parc_mopt_set_params(ParcMotionOpt *h, const float *params_host);      /* [F][NP]; resets Adam */
int parc_mopt_get_params(ParcMotionOpt *h, float *params_host);
/* Loss terms [num_clips][9] and the gradient of the weighted total [F][NP] at the current iterate (either may be NULL). */
int parc_mopt_loss_and_grad(ParcMotionOpt *h, float *terms_host, float *grad_host);
/* n_iters Adam iterations; terms_host (may be NULL) receives [n_iters][num_clips][9], the terms each iteration's gradient came from. */
int parc_mopt_step(ParcMotionOpt *h, int32_t n_iters, float *terms_host);
/* The optimised frames: root_pos [F][3], root_rot [F][4] (exp_map_to_quat), joint_rot [F][B-1][4] (dof_to_rot). */
int parc_mopt_get_frames(ParcMotionOpt *h, float *root_pos_host, float *root_rot_host, float *joint_rot_host);
/* FK of the SOURCE frames: body_pos [F][B][3], body_rot [F][B][4]. */
int parc_mopt_get_source_body(ParcMotionOpt *h, float *body_pos_host, float *body_rot_host);
/* compute_approx_body_constraints' refinement: n points, each on the full terrain of clip clip_host[i], `steps` SGD steps of
 * lr on sdf^2 (non-inverted, base_z = min(hf) - 10), one lane per point and one launch per step; points updated in place. */
int parc_mopt_build_constraints(ParcMotionOpt *h, int32_t n, const int32_t *clip_host, float *points_host, int32_t steps, float lr);
/* Per-kernel device time (hipEvents) of the last parc_mopt_step call, ms per iteration: fk, patch, points, grad, reduce, adam. */
int parc_mopt_kernel_times(ParcMotionOpt *h, float *ms6);

/* The motion generator's training loss: the reference's MDM.motion_difference (motion_generator/mdm.py:573-692) for
 * N windows of T frames in one launch, with the analytic derivative of each window's sum of terms with respect to the standardised
 * prediction (through unstandardise, exp_map_to_quat, joint_dof_to_rot and forward kinematics).  Its own handle; every array of a call
 * is a device pointer and the launch goes to the caller's stream.  A prediction row is root_pos[3] | root exp map[3] | joint
 * positions[3 (B - 1)] | joint dofs[dof_size] | contacts[B].  Terms, in this order: VEL_ROOT_POS, VEL_ROOT_ROT, VEL_JOINT_ROT,
 * SIMPLE_ROOT_POS, SIMPLE_ROOT_ROT, SIMPLE_JOINT_ROT, SIMPLE_CONTACT, SIMPLE_BODY_POS, FK_BODY_POS, FK_BODY_ROT, BODY_POS_CONSISTENCY,
 * VEL_FK_BODY_POS, TARGET.  A window's result does not depend on which other windows are in the batch. */
#define PARC_MLOSS_NUM_TERMS 13
#define PARC_MLOSS_SQUARED_L2 0
#define PARC_MLOSS_PSEUDO_HUBER 1
typedef struct ParcMotionLoss ParcMotionLoss;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionLossParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    float sequence_fps;                      /* velocities are differences of neighbouring frames times this */
    int32_t num_prev_states;                 /* >= 1: the target term measures from frame num_prev_states - 1 to the last frame */
    float weights[PARC_MLOSS_NUM_TERMS];     /* in the order of the terms */
    int32_t use_pos_loss;                    /* 0: the four FK terms (FK_BODY_POS, FK_BODY_ROT, BODY_POS_CONSISTENCY, VEL_FK_BODY_POS) are 0 */
    int32_t use_target_loss;                 /* 0: TARGET is 0 and target_dir is not read */
    float target_dir_len_eps;                /* TARGET = w clamp(-dir . (root_xy[T - 1] - root_xy[num_prev_states - 1]), min = -eps) */
    int32_t loss_fn;                         /* PARC_MLOSS_SQUARED_L2: sum of squares; PARC_MLOSS_PSEUDO_HUBER: sqrt(sum(sq + 0.0009)) - 0.03 */
} ParcMotionLossParams;
typedef struct {
    int32_t n, num_frames;                   /* N >= 1 windows of T >= 2 frames, T >= num_prev_states */
    const float *pred;                       /* [N][T][D] standardised */
    const float *mean, *std;                 /* [T][D] */
    const float *root_pos, *root_rot, *joint_rot, *contacts;   /* the true windows: [N][T][3], [N][T][4] xyzw, [N][T][B-1][4], [N][T][B] */
    const float *target_dir;                 /* [N][2]; may be NULL without use_target_loss */
    float *terms;                            /* out [N][PARC_MLOSS_NUM_TERMS]: the weighted value of every term per window */
    float *grad;                             /* out [N][T][D]: d (the window's sum of terms) / d pred */
} ParcMotionLossArgs;
int parc_mloss_create(const ParcMotionLossParams *p, ParcMotionLoss **out);
void parc_mloss_destroy(ParcMotionLoss *h);
/* One launch on `stream`, no host synchronisation (but when the workspace has to grow to a larger N x T than any call before). */
int parc_mloss_eval(ParcMotionLoss *h, const ParcMotionLossArgs *a, void *stream);
/* Device time (hipEvents) of the last parc_mloss_eval, ms; synchronises with it. */
int parc_mloss_kernel_times(ParcMotionLoss *h, float *ms1);

/* Motion-terrain analysis for B clips at once, each on its own terrain: the reference's
 * terrain_util.compute_hf_extra_vals (per-frame heightfield cell masks, lowest body point per cell, augmentation bounds hf_maxmin,
 * terrain_util.py:1851-1947), mdm_path.compute_motion_loss with unit weights (penetration and contact against the exact column-box
 * SDF of the whole terrain, mdm_path.py:31-127) and the jerk statistics of scripts/motion_tests/compute_losses.py:163-174.
 * Its own handle.  The clips use the optimiser's layout (ParcMotionOptClips; the constraint fields are ignored).  A frame whose inputs
 * or sample points are not finite contributes no cells and no heights and makes its clip's scores and max root z NaN; other clips are
 * unaffected.  Results do not depend on which other clips are in the batch. */
#define PARC_MTERR_SDF_PRUNED 0                  /* exact ring-pruned search of the whole terrain (default) */
#define PARC_MTERR_SDF_BRUTE 1                   /* every cell for every point (bit-identical to the pruned search; for tests) */
#define PARC_MTERR_CLIP_OUTPUTS 6                /* pen_loss, contact_loss, mean_jerk, jerk_frac, max_root_z, min_hf */
typedef struct ParcMotionTerrain ParcMotionTerrain;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionTerrainParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t num_points;                      /* sample points per frame, [1, PARC_MOPT_MAX_POINTS]; contiguous per body, bodies in order */
    const float *points_host;                /* [num_points][3] body-local */
    const int32_t *point_body_host;          /* [num_points] */
    int32_t contact_body_id[PARC_MAX_BODIES];/* column of the contacts array of each body, -1 = not scored (compute_motion_loss: b -> b) */
    double z_buf;                            /* hf_maxmin default bounds: max root z + z_buf, min hf - z_buf (reference default 3.0) */
    double jump_buf;                         /* jump cells: lowest point - hf >= jump_buf (fp32), bound lowest point - jump_buf (0.8) */
    double max_jerk;                         /* jerk_frac threshold, compared in fp32 (compute_losses.py: 11666.3906) */
    int32_t sdf_mode;                        /* PARC_MTERR_SDF_* */
} ParcMotionTerrainParams;
int parc_mterr_create(const ParcMotionTerrainParams *p, ParcMotionTerrain **out);
void parc_mterr_destroy(ParcMotionTerrain *h);
/* Uploads the clips (num_clips >= 1, every clip >= 1 frame, dims >= 1 with at most 2^31 - 1 cells, dx > 0).  As parc_mopt_set_clips:
 * PARC_ERR_INVALID leaves the batch loaded before in place and usable, with its last run's results; a failure after the validation
 * leaves no batch (PARC_ERR_STATE until a parc_mterr_set_clips succeeds). */
int parc_mterr_set_clips(ParcMotionTerrain *h, const ParcMotionOptClips *c);
/* One analysis of the uploaded clips.  Outputs (NULL = not copied): clip_out [num_clips][PARC_MTERR_CLIP_OUTPUTS]; mask_counts [F], the
 * number of distinct cells of each frame; hf_maxmin [cells][2] (max, min), cells in hf_host's order; total_inds = sum of mask_counts.
 * mean_jerk / jerk_frac are NaN for clips of fewer than 4 frames; jerk_frac divides by frames - 3, not by samples (the reference's). */
int parc_mterr_run(ParcMotionTerrain *h, float *clip_out_host, int32_t *mask_counts_host, float *hf_maxmin_host, int64_t *total_inds);
/* The cells of the last run: int32 [total_inds][2] (i, j), frames in order, each frame's cells in lexicographic order without repeats. */
int parc_mterr_get_mask_inds(ParcMotionTerrain *h, int32_t *inds_host);
/* TEST entry: the lowest body point per cell of the last run ([cells], 99999.9999f where untouched) and the touched flags ([cells]). */
int parc_mterr_get_min_heights(ParcMotionTerrain *h, float *min_heights_host, int32_t *touched_host);
/* TEST entry: the raw ground / air SDF minima [num_frames][num_points] of frames [frame0, frame0 + num_frames) (after a run). */
int parc_mterr_point_sdf(ParcMotionTerrain *h, int64_t frame0, int32_t num_frames, float *ground_host, float *air_host);
/* Device time (hipEvents) of the last run, ms: fk, init, points, reduce, cells, and gather (the last parc_mterr_get_mask_inds). */
int parc_mterr_kernel_times(ParcMotionTerrain *h, float *ms6);

/* Motion-window sampler for generator training: the reference's MDMHeightfieldContactMotionSampler
 * (mdm_heightfield_contact_motion_sampler.py) for a whole batch.  Its own handle.  Per sample: a window of T frames at t0 + times[k]
 * (calc_motion_frame), canonicalised to the heading frame of frame ref_frame and run through FK; the target (root at t_future, in that
 * frame); the local Gx x Gy heightfield around the reference root with the per-window augmentation bounds (the clip's hf_maxmin where the
 * window's hf_mask_inds touch a cell, (2 max_h, -2 max_h) elsewhere) and the terrain augmentation.  Every random value comes from a plan
 * (device arrays of derived values); parc_msamp_draw_plan fills one from a seed with the counter-based generator.  A sample's outputs
 * do not depend on the batch it is in or on its position.  Limits: T <= PARC_MSAMP_MAX_FRAMES, patch sides <= PARC_MSAMP_MAX_GRID,
 * a clip's terrain <= PARC_MSAMP_MAX_TERRAIN_CELLS cells (the window mask is a bitset in LDS), max_num_boxes <= PARC_MSAMP_MAX_BOXES. */
#define PARC_MSAMP_MAX_FRAMES 64
#define PARC_MSAMP_MAX_GRID 32
#define PARC_MSAMP_MAX_TERRAIN_CELLS (512 * 512)
#define PARC_MSAMP_MAX_BOXES 64
#define PARC_MSAMP_BOX_FLOATS 6                  /* center x, y (patch index units), len x, y, angle, height */
#define PARC_MSAMP_RELATIVE_TO_ROOT 0            /* RelativeZStyle */
#define PARC_MSAMP_RELATIVE_TO_ROOT_FLOOR 1
#define PARC_MSAMP_AUG_NOISE 0                   /* HFAugmentationMode */
#define PARC_MSAMP_AUG_MAXPOOL_AND_BOXES 1
#define PARC_MSAMP_AUG_NONE 2
#define PARC_MSAMP_POOL_NONE 0                   /* plan pool_kind: maxpool_hf, maxpool_hf_1d_x, maxpool_hf_1d_y */
#define PARC_MSAMP_POOL_2D 1
#define PARC_MSAMP_POOL_1D_X 2
#define PARC_MSAMP_POOL_1D_Y 3
#define PARC_MSAMP_STATUS_BAD_MOTION 1           /* plan status bits (parc_msamp_plan_status) */
#define PARC_MSAMP_STATUS_BAD_BOXES 2
#define PARC_MSAMP_STATUS_BAD_POOL 4
typedef struct ParcMotionSampler ParcMotionSampler;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionSamplerParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t num_frames;                      /* T = len(arange(0, sequence_duration, 1 / sequence_fps)) */
    const float *times_host;                 /* [T] that arange, fp32 */
    float timestep;                          /* fp32(1 / sequence_fps): the frame index of a window is round(t0 / timestep) */
    float sequence_duration;
    int32_t ref_frame;                       /* num_prev_states - 1 */
    int32_t autoregressive;                  /* 0: drawn start times are 0 */
    int32_t relative_z_style;                /* PARC_MSAMP_RELATIVE_* */
    int32_t aug_mode;                        /* PARC_MSAMP_AUG_* (use_hf_augmentation = false is AUG_NONE) */
    int32_t grid_dim_x, grid_dim_y;          /* Gx = num_x_neg + 1 + num_x_pos, Gy likewise */
    int32_t num_x_neg, num_y_neg;
    const float *grid_x_host, *grid_y_host;  /* [Gx], [Gy]: get_xy_grid_points' linspace values around 0 */
    float grid_min_x, grid_min_y;            /* fp32(-num_neg) * fp32(dx) (floor heights) */
    float dx;                                /* heightmap.horizontal_scale */
    float max_h;
    int32_t max_num_boxes;
    float box_min_len, box_max_len;
    float hf_maxpool_chance;
    int32_t hf_max_maxpool_size;
    float hf_change_height_chance;
    float future_pos_noise_scale, future_window_min, future_window_max;
} ParcMotionSamplerParams;
typedef struct {                             /* with ParcMotionOptClips (constraint fields ignored) */
    const float *hf_maxmin_host;             /* [cells][2] (max, min), cells in hf_host's order */
    const int64_t *mask_off_host;            /* [F + 1] CSR offsets of the frames' hf_mask_inds, frames in clip order */
    const int32_t *mask_cells_host;          /* [mask_off[F]] cell i * Y + j */
    const int32_t *fps_host;                 /* [num_clips] */
    const int32_t *loop_modes_host;          /* [num_clips] PARC_LOOP_* */
    const double *weights_host;              /* [num_clips] sampling weights (normalised on load) */
} ParcMotionSamplerClipInfo;
typedef struct {                             /* device arrays of n samples; derived values, not uniforms */
    int32_t n;
    const int32_t *motion_id;                /* [n] */
    const float *t0, *t_future;              /* [n] */
    const float *future_pos_noise;           /* [n][3] already scaled */
    const int32_t *change_height;            /* [n] */
    const float *height_value;               /* [n] */
    const int32_t *pool_kind, *pool_size;    /* [n][3] PARC_MSAMP_POOL_* in application order; half widths >= 0 */
    const int32_t *num_boxes;                /* [n] in [0, max_num_boxes] */
    const float *boxes;                      /* [n][max_num_boxes][PARC_MSAMP_BOX_FLOATS] */
    const float *noise;                      /* [n][Gx][Gy] the noisy heightfield of AUG_NOISE (NULL in the other modes) */
} ParcMotionSamplerPlan;
typedef struct {                             /* caller-owned device buffers; NULL = not written */
    float *root_pos, *root_rot;              /* [n][T][3], [n][T][4] */
    float *joint_pos, *joint_rot;            /* [n][T][B-1][3] body positions without the root, [n][T][B-1][4] */
    float *contacts;                         /* [n][T][B] */
    float *floor_heights;                    /* [n][T] (needs root_pos and hfs) */
    float *hfs;                              /* [n][Gx][Gy] */
    float *target_pos, *target_rot;          /* [n][3], [n][4] */
    float *hf_bounds;                        /* [n][Gx][Gy][2] the per-window (max, min) after the relative-z shift (tests) */
} ParcMotionSamplerOutputs;
int parc_msamp_create(const ParcMotionSamplerParams *p, ParcMotionSampler **out);
void parc_msamp_destroy(ParcMotionSampler *h);
/* Uploads the library.  PARC_ERR_INVALID names the clip (by index) that has no full window (num_frames - T <= 0) or whose terrain has
 * more than PARC_MSAMP_MAX_TERRAIN_CELLS cells.  As parc_mopt_set_clips: PARC_ERR_INVALID leaves the library loaded before in place and
 * usable; a failure after the validation leaves no library, never part of one (PARC_ERR_STATE until a parc_msamp_set_clips succeeds). */
int parc_msamp_set_clips(ParcMotionSampler *h, const ParcMotionOptClips *c, const ParcMotionSamplerClipInfo *info);
/* The deterministic path: everything is enqueued on `stream`, no host sync. */
int parc_msamp_sample_with(ParcMotionSampler *h, const ParcMotionSamplerPlan *plan, const ParcMotionSamplerOutputs *out, void *stream);
/* Fills the (writable, caller-owned) arrays of `plan` for plan->n samples from `seed` (Philox4x32-10, counter = sample index). */
int parc_msamp_draw_plan(ParcMotionSampler *h, uint64_t seed, const ParcMotionSamplerPlan *plan, void *stream);
/* draw_plan + sample_with. */
int parc_msamp_sample(ParcMotionSampler *h, uint64_t seed, const ParcMotionSamplerPlan *plan, const ParcMotionSamplerOutputs *out, void *stream);
/* get_motion_sequences_for_id: the num_frames - T windows of clip `clip` starting at frames 0, 1, ... (t0 = frame * fp32(1/fps)); motion
 * outputs only (hfs, floor_heights, targets and bounds must be NULL). */
int parc_msamp_enumerate(ParcMotionSampler *h, int32_t clip, const ParcMotionSamplerOutputs *out, void *stream);
/* Synchronises `stream` and returns the OR of the PARC_MSAMP_STATUS_* bits the kernels raised since the last call (then cleared).
 * A sample with a bad plan entry is still computed memory-safely (ids and counts clamped) but its values are not meaningful. */
int parc_msamp_plan_status(ParcMotionSampler *h, void *stream, int32_t *status);
/* Device time (hipEvents; waits for the last event) of the last sample_with / sample call, ms: draw (0 for sample_with), window,
 * heightfield. */
int parc_msamp_kernel_times(ParcMotionSampler *h, float *ms3);

/* Batched terrain path planner: stage 2's A* search (motion_synthesis/procgen/astar.py, driven as
 * scripts/parc_2_kin_gen.py:310-337) for Q queries at once, each its own dim_x x dim_y heightfield, start cell and goal cell.  Its own
 * handle.  Per query: the optional terrain simplification (flat_maxpool_2x2, then flatten_4x4_near_edge around the start and around the
 * goal), the navigation graph (8 neighbours within max_z_diff; jump edges between cliff cells with a Bresenham line of sight), the
 * search, the node list and the 3-D polyline of run_a_star_on_start_end_nodes.  All of it fp32 in the reference's association.
 * The pop order is the contract (the metre heuristic is not admissible against squared-metre step costs): the open cell with the smallest
 * (f, g) is popped; a tie on (f, g) between different cells goes to the LOWEST CELL INDEX i * dim_y + j (the reference's comparison of
 * tied nodes is not a total order).  Two stated differences from the reference:
 *   - step-cost noise: not a global stream consumed in expansion order but a pure function of (seed, query index, from cell, to cell):
 *     Philox4x32-10 keyed by the seed, counter (hi = query index, lo = from << 16 | to), u = the first word's top 24 bits / 2^24,
 *     noise = fp32(u * fp32(uniform_cost_max - uniform_cost_min) + fp32(uniform_cost_min)), added last;
 *   - max_compute_time (wall clock) becomes max_expansions: a query that would pop more cells ends with PARC_PATHPLAN_BUDGET and
 *     counts as a failure (the reference returns the path to whatever node it was at).
 * Start / goal cells are injected by the caller or drawn on the device: both uniform over pick_random_start_end_nodes_on_edges'
 * candidate list (i in {1, 2, X-3, X-2} or j in {1, 2, Y-3, Y-2}), redrawn until their xy distance is >= min_start_end_xy_dist - 1e-4;
 * draw t of query q uses counter (hi = 1 << 62 | q, lo = t), words 0 and 1, index = min(int(u * n), n - 1); after 1000 draws the query
 * ends with PARC_PATHPLAN_NO_DRAW (the reference asserts).  The query index is first_query + the position in the batch, so a query
 * computes the same bits alone or in any batch.  Limits: sides of 4 .. PARC_PATHPLAN_MAX_DIM cells (a query's search state lives in LDS:
 * 14 B per cell, 57.9 KB at 64 x 64), jump window radius ceil(max_jump_xy_dist / dx) <= PARC_PATHPLAN_MAX_JUMP_RADIUS. */
#define PARC_PATHPLAN_MAX_DIM 64
#define PARC_PATHPLAN_MAX_JUMP_RADIUS 8
#define PARC_PATHPLAN_JUMP_WORDS 8               /* (2 * PARC_PATHPLAN_MAX_JUMP_RADIUS)^2 window candidates / 32 */
#define PARC_PATHPLAN_FOUND 0
#define PARC_PATHPLAN_NO_PATH 1                  /* the open set ran empty */
#define PARC_PATHPLAN_OVER_MAX_COST 2            /* a path exists (cost and nodes are returned) but cost > max_cost */
#define PARC_PATHPLAN_BUDGET 3                   /* more than max_expansions pops */
#define PARC_PATHPLAN_NO_DRAW 4                  /* no start / goal pair far enough apart in 1000 draws */
typedef struct ParcPathPlanner ParcPathPlanner;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcPathPlanParams) */
    int32_t device;
    int32_t dim_x, dim_y;                    /* one grid shape per handle */
    float dx, dy;                            /* SubTerrain.dxdy */
    float min_point[2];                      /* SubTerrain.min_point (stage 2: 0, 0) */
    /* AStarSettings (astar.py:12-24), Python floats */
    double max_z_diff, max_jump_xy_dist, max_jump_z_diff, min_jump_z_diff, w_z, w_xy, w_bumpy, max_bumpy;
    double uniform_cost_max, uniform_cost_min, min_start_end_xy_dist, max_cost;
    int32_t simplify_terrain;                /* parc_2_kin_gen's simplify_terrain */
    int32_t max_expansions;                  /* pops per query before PARC_PATHPLAN_BUDGET */
    int32_t max_nodes, max_points;           /* row lengths of the node and polyline outputs */
} ParcPathPlanParams;
typedef struct {                             /* host arrays of Q entries; NULL = not copied */
    int32_t *status;                         /* [Q] PARC_PATHPLAN_* */
    float *cost;                             /* [Q] g of the goal (NaN unless FOUND / OVER_MAX_COST) */
    int32_t *num_nodes;                      /* [Q] cells of the path, start and goal included (may exceed max_nodes: then cut) */
    int32_t *nodes;                          /* [Q][max_nodes] cell index i * dim_y + j */
    int32_t *num_points;                     /* [Q] polyline points of a FOUND query (may exceed max_points: then cut) */
    float *points;                           /* [Q][max_points][3] */
    int32_t *start, *goal;                   /* [Q][2] the cells used */
    float *hf;                               /* [Q][dim_x][dim_y] the heightfield searched (simplified when simplify_terrain) */
    int32_t *pops;                           /* [Q] */
} ParcPathPlanOutputs;
int parc_pathplan_create(const ParcPathPlanParams *p, ParcPathPlanner **out);
void parc_pathplan_destroy(ParcPathPlanner *h);
/* Plans Q queries: hf_host [Q][dim_x][dim_y]; start_host / goal_host [Q][2] cells, or both NULL to draw them from (seed, query index).
 * Synchronous (the outputs are host arrays).  The device buffers are kept from run to run and replaced when Q exceeds what they hold (the
 * old ones released first).  PARC_ERR_INVALID leaves the last batch readable by parc_pathplan_get_graph; a later failure leaves none
 * (PARC_ERR_STATE there until a run succeeds), and a failed allocation leaves no buffers either: the next run allocates them anew. */
int parc_pathplan_run(ParcPathPlanner *h, int32_t Q, const float *hf_host, const int32_t *start_host, const int32_t *goal_host, uint64_t seed,
                      uint64_t first_query, const ParcPathPlanOutputs *out);
/* The navigation graph of queries [q0, q0 + n) of the last run, from the predicates the search uses: nbr [n][cells] bit d = the edge to
 * neighbour d of (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (-1,1) (1,-1) (1,1); cliff [n][cells]; jump [n][cells][PARC_PATHPLAN_JUMP_WORDS],
 * bit k = the jump edge from (i, j) to (i - R + k / 2R, j - R + k % 2R), R the jump window radius. */
int parc_pathplan_get_graph(ParcPathPlanner *h, int32_t q0, int32_t n, uint8_t *nbr_host, uint8_t *cliff_host, uint32_t *jump_host);
/* Device time (hipEvents) of the last run, ms: prepare (draw + simplification), search, and the last parc_pathplan_get_graph. */
int parc_pathplan_kernel_times(ParcPathPlanner *h, float *ms3);

/* Batched procedural terrain generator: stage 2's BOXES, PATHS and STAIRS procgen modes (terrain_util's
 * add_boxes_to_hf2 without the hf_maxmin clamp, gen_paths_hf, add_stairs_to_hf / draw_box, driven as scripts/parc_2_kin_gen.py:247-290)
 * for n terrains at once, one wave per terrain.  Its own handle: one mode and one grid shape per handle.  Every random value comes from
 * a plan of device arrays holding the derived fp32 values (not the uniforms); parc_tgen_draw_plan fills one with Philox4x32-10 keyed by
 * the seed, counter hi = 1 << 61 | mode << 56 | terrain index, u = top 24 bits / 2^24, normals by Box-Muller on (0, 1] uniforms:
 *   BOXES   lo = 2 b: center x, y, len x, y of box b; lo = 2 b + 1: angle, height
 *   PATHS   lo = 256 p: start x, y, angle, height of path p; 256 p + 1: vy; 256 p + 2 + i / 4: turn normals 4 (i / 4) .. 4 (i / 4) + 3
 *           (r0 cos, r0 sin, r1 cos, r1 sin of the uniform pairs (0, 1) and (2, 3))
 *   STAIRS  lo = 2 s: start x, y, end x, y of stair s; lo = 2 s + 1: start height, step height, thickness
 * The terrain index is first_terrain + the position in the batch: a terrain is the same bits alone or in any batch.  Limits (a refusal
 * names the macro): sides of 4 .. PARC_TGEN_MAX_DIM cells, num_boxes <= PARC_TGEN_MAX_BOXES, num_terrain_paths <= PARC_TGEN_MAX_PATHS (a
 * lane per path), num_stairs <= PARC_TGEN_MAX_STAIRS, maxpool_size <= PARC_TGEN_MAX_POOL; a path has PARC_TGEN_PATH_POINTS points; a stair
 * paints at most PARC_TGEN_MAX_STEPS steps (a plan whose stair would need more is cut there; the validate pass refuses it). */
#define PARC_TGEN_MAX_DIM 64
#define PARC_TGEN_MAX_BOXES 64
#define PARC_TGEN_MAX_PATHS 64
#define PARC_TGEN_MAX_STAIRS 16
#define PARC_TGEN_MAX_POOL 8
#define PARC_TGEN_PATH_POINTS 1000
#define PARC_TGEN_MAX_STEPS 1024
#define PARC_TGEN_BOX_FLOATS 6                   /* center x, y (index units), len x, y, angle, height: PARC_MSAMP_BOX_FLOATS' layout */
#define PARC_TGEN_STAIR_FLOATS 7                 /* start x, y, end x, y (metres), start height, step height, thickness */
#define PARC_TGEN_BOXES 0                        /* ProcGenMode (parc_2_kin_gen.py:30-34) */
#define PARC_TGEN_PATHS 1
#define PARC_TGEN_STAIRS 2
typedef struct ParcTerrainGen ParcTerrainGen;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcTerrainGenParams) */
    int32_t device;
    int32_t mode;                            /* PARC_TGEN_BOXES / PATHS / STAIRS */
    int32_t dim_x, dim_y;
    float dx, dy;                            /* SubTerrain.dxdy */
    float min_point[2];                      /* SubTerrain.min_point (stage 2: 0, 0) */
    /* the ranges parc_tgen_draw_plan draws from: ProcGenBoxesSettings, ProcGenPathsSettings, ProcGenStairsSettings */
    int32_t num_boxes;
    float min_box_h, max_box_h, box_min_len, box_max_len, min_box_angle, max_box_angle;
    int32_t num_terrain_paths, maxpool_size;
    float path_min_height, path_max_height, floor_height;
    int32_t num_stairs;
    float min_stair_start_height, max_stair_start_height, min_step_height, max_step_height, min_stair_thickness, max_stair_thickness;
} ParcTerrainGenParams;
typedef struct {                             /* device arrays of n terrains; only the handle's mode is read (the others may be NULL) */
    int32_t n;
    const float *boxes;                      /* [n][num_boxes][PARC_TGEN_BOX_FLOATS] */
    const float *path_start;                 /* [n][num_terrain_paths][2] metres */
    const float *path_vy;                    /* [n][num_terrain_paths] the start velocity is (1, vy) rotated by path_angle */
    const float *path_angle;                 /* [n][num_terrain_paths] */
    const float *path_turn;                  /* [n][num_terrain_paths][PARC_TGEN_PATH_POINTS] standard normals */
    const float *path_height;                /* [n][num_terrain_paths] */
    const float *stairs;                     /* [n][num_stairs][PARC_TGEN_STAIR_FLOATS] */
} ParcTerrainGenPlan;
int parc_tgen_create(const ParcTerrainGenParams *p, ParcTerrainGen **out);
void parc_tgen_destroy(ParcTerrainGen *h);
/* Fills the (writable, caller-owned) arrays of `plan` for plan->n terrains from (seed, first_terrain + position).  No host sync. */
int parc_tgen_draw_plan(ParcTerrainGen *h, uint64_t seed, uint64_t first_terrain, const ParcTerrainGenPlan *plan, void *stream);
/* The deterministic path: hf [n][dim_x][dim_y] (device) from the plan.  With validate != 0 a pass over the plan runs first and the
 * call synchronises: a non-finite entry, or a stair of more than PARC_TGEN_MAX_STEPS steps, is PARC_ERR_INVALID naming the field, and the
 * generator is not launched.  Without it nothing synchronises; a non-finite entry is handled memory-safely (indices clamp to the grid). */
int parc_tgen_generate_with(ParcTerrainGen *h, const ParcTerrainGenPlan *plan, float *hf, int32_t validate, void *stream);
/* draw_plan + generate_with in one kernel, the plan never in memory: the same bits as the two calls. */
int parc_tgen_generate(ParcTerrainGen *h, int32_t n, uint64_t seed, uint64_t first_terrain, float *hf, void *stream);
/* Device time (hipEvents; waits for the last event), ms: the last parc_tgen_draw_plan, the last generate_with / generate (0 = not run). */
int parc_tgen_kernel_times(ParcTerrainGen *h, float *ms2);

/* Batched motion-terrain augmenter: scripts/run_simple_augment_motions.py:144-202 (window, heading, x / y scale,
 * SubTerrain.pad, slice_terrain_around_motion, HEIGHT_SCALE / BOXES_ALONG_PATH) and stage 2's mirrored copies (parc_2_kin_gen.py:490-495:
 * flip_motion_about_XZ_plane, flip_by_XZ_axis) for n variations at once.  Its own handle.  The source clips use the optimiser's layout
 * (ParcMotionOptClips; the constraint fields are ignored).  Every random value comes from a plan of device arrays holding the derived
 * values (not the uniforms); parc_maug_draw_plan fills one with Philox4x32-10 keyed by the seed, counter hi = 1 << 62 | variation index,
 * u = top 24 bits / 2^24:
 *   lo = 0      source clip (inverse CDF of the sample weights), start frame, heading
 *   lo = 1      x scale, y scale, height scale (uniform on [min_h_scale, max_h_scale] minus the open bad_h_range), box count
 *   lo = 2 + 2b frame, len x, len y, angle of box b;  lo = 3 + 2b: its height
 * The variation index is first_variation + the position in the batch: a variation is the same bits alone or in any batch.  The variations
 * of a run differ in frame count and slice size: the results stay in the handle, concatenated, until the next run, and
 * parc_maug_get_result copies them out.  A slice may have at most PARC_MAUG_MAX_DIM cells a side (a refusal names the macro). */
#define PARC_MAUG_MAX_DIM 128
#define PARC_MAUG_MAX_BOXES 16
#define PARC_MAUG_BOX_FLOATS 4                   /* len x, len y (cells), angle, height; the centre is the box's frame */
#define PARC_MAUG_HEIGHT_SCALE 0                 /* TerrainAugmentationType (run_simple_augment_motions.py:19-22) */
#define PARC_MAUG_BOXES_ALONG_PATH 1
#define PARC_MAUG_NONE 2
#define PARC_MAUG_STATUS_CLAMPED 1               /* parc_maug_plan_status: a plan index lay outside its range and was clamped */
#define PARC_MAUG_STATUS_NOT_FINITE 2            /* a variation's bounds were NaN or infinite: its slice is 1 x 1 */
typedef struct ParcMotionAug ParcMotionAug;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionAugParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t joint_swap[PARC_MAX_BODIES];     /* the left / right partner of every joint (by name), itself when it has none */
    int32_t contact_swap[PARC_MAX_BODIES];   /* the same for the columns of the contacts array */
    int32_t mode;                            /* PARC_MAUG_HEIGHT_SCALE / BOXES_ALONG_PATH / NONE */
    int32_t terrain_padding_size;            /* cells of SubTerrain.pad on every side (0: none) */
    int32_t slice_terrain;                   /* 0: the (padded) terrain and the frames keep their place (what the mirrored copies use) */
    int32_t sample_weight_by_length;         /* parc_maug_draw_plan: clips weighted by frames / fps, else uniformly */
    float min_heading_angle, max_heading_angle;   /* degrees */
    float x_scale[2], y_scale[2];
    float min_h_scale, max_h_scale, bad_h_range[2];
    int32_t min_num_boxes, max_num_boxes;
    float min_len, max_len, min_angle, max_angle, min_h, max_h;
} ParcMotionAugParams;
typedef struct {                             /* with ParcMotionOptClips */
    const float *hf_maxmin_host;             /* [cells][2] (max, min), or NULL: no hf_maxmin output */
    const int32_t *fps_host;                 /* [num_clips] */
    const int32_t *max_frames_host;          /* [num_clips] int(round(fps * max_motion_len)): the longest window parc_maug_draw_plan cuts */
} ParcMotionAugClipInfo;
typedef struct {                             /* device arrays of n variations; every array is required */
    int32_t n;
    const int32_t *src_clip, *start_frame, *num_frames;   /* [n] */
    const float *heading;                    /* [n] radians */
    const float *scale;                      /* [n][2] x, y */
    const int32_t *mirror;                   /* [n] 0 / 1 */
    const float *height_scale;               /* [n] (HEIGHT_SCALE) */
    const int32_t *num_boxes;                /* [n] <= PARC_MAUG_MAX_BOXES (BOXES_ALONG_PATH) */
    const int32_t *box_frame;                /* [n][PARC_MAUG_MAX_BOXES] frame of the window under which box b sits */
    const float *boxes;                      /* [n][PARC_MAUG_MAX_BOXES][PARC_MAUG_BOX_FLOATS] */
} ParcMotionAugPlan;
typedef struct { int32_t n, has_maxmin; int64_t total_frames, total_cells; } ParcMotionAugSizes;
typedef struct {                             /* device arrays owned by the caller; a NULL one is not copied */
    int64_t *frame_off, *cell_off;           /* [n + 1] */
    int32_t *src_clip;                       /* [n] */
    int32_t *hf_dims;                        /* [n][2] */
    float *hf_geom;                          /* [n][4] min_x, min_y, dx, dy */
    float *canon_z;                          /* [n] the height that was under frame 0 */
    float *root_pos, *root_rot, *joint_rot, *contacts;   /* [F][3], [F][4] xyzw, [F][B-1][4], [F][B] */
    float *hf;                               /* [cells], x-major per variation */
    float *hf_maxmin;                        /* [cells][2] */
} ParcMotionAugOutputs;
int parc_maug_create(const ParcMotionAugParams *p, ParcMotionAug **out);
void parc_maug_destroy(ParcMotionAug *h);
/* Validates and uploads the source clips (as parc_msamp_set_clips: an invalid batch leaves the loaded one in place). */
int parc_maug_set_clips(ParcMotionAug *h, const ParcMotionOptClips *c, const ParcMotionAugClipInfo *info);
/* Fills the (writable, caller-owned) arrays of `plan` for plan->n variations from (seed, first_variation + position); every
 * variation gets the mirror flag `mirror`.  No host sync.  The struct is the readers' (const members); this call alone writes through them. */
int parc_maug_draw_plan(ParcMotionAug *h, uint64_t seed, uint64_t first_variation, int32_t mirror, const ParcMotionAugPlan *plan, void *stream);
/* The deterministic path.  Synchronises twice on small copies (the frame total, the slice dims).  With validate != 0 a pass over the plan
 * runs first: a non-finite or out-of-range entry is PARC_ERR_INVALID naming the field, and nothing is launched.  Without it a bad index is
 * clamped into its range (parc_maug_plan_status reports that) and a NaN or infinite heading or scale stays inside its own variation (a
 * 1 x 1 slice); a finite scale so large that the slice passes PARC_MAUG_MAX_DIM is that refusal, and refuses the run. */
int parc_maug_augment_with(ParcMotionAug *h, const ParcMotionAugPlan *plan, int32_t validate, void *stream, ParcMotionAugSizes *sizes);
/* draw_plan + augment_with without the plan in memory: the same bits as the two calls. */
int parc_maug_augment(ParcMotionAug *h, int32_t n, uint64_t seed, uint64_t first_variation, int32_t mirror, void *stream, ParcMotionAugSizes *sizes);
/* Copies the last run's results (device to device, on `stream`) into the arrays of `out`, sized by that run's ParcMotionAugSizes. */
int parc_maug_get_result(ParcMotionAug *h, const ParcMotionAugOutputs *out, void *stream);
/* Synchronises; the OR of PARC_MAUG_STATUS_* since the last call, then clears it. */
int parc_maug_plan_status(ParcMotionAug *h, void *stream, int32_t *status);
/* Device time (hipEvents; waits for the last event), ms: the last draw_plan, then layout + scan, frames + scan, terrain of the last run. */
int parc_maug_kernel_times(ParcMotionAug *h, float *ms4);

/* ---- motion generator inference: the MDM denoiser and its reverse-diffusion loop (parc_mdm_*) ------------------
 * Inference of the reference's MDMTransformer (motion_generator/mdm_transformer.py) in eval mode and fp32, with the sampling loops of
 * motion_generator/mdm.py (ddim_inference :932, reverse_diffusion :855, predict_x0 :836, project_dofs :990).  Three kernels:
 * k_mdm_cond (embed_conds, once per generation), k_mdm_forward (one workgroup per sample from tokens to x_0; with guidance both passes
 * of a step are one launch over 2 B rows) and k_mdm_update (guidance combine, project_dofs, the DDIM / DDPM step).  A sample's result
 * does not depend on its batch.  Shapes outside the limits below are refused by parc_mdm_create, never computed. */
#define PARC_MDM_MAX_LAYERS 8
#define PARC_MDM_MAX_HIDDEN 8                    /* hidden widths of one MLP list */
#define PARC_MDM_MAX_WIDTH 1024                  /* an MLP hidden width */
#define PARC_MDM_MAX_DIM 512                     /* d_hid (a multiple of 16) */
#define PARC_MDM_MAX_D_MODEL 416                 /* d_model (a multiple of 16): the residual stream [tokens][d_model + 4] and the score tiles share 160 KB
                                                  * of LDS, so the limit falls with seq_len: 416 at 1 frame, 352 at 15, 208 at 64; create names the bytes */
#define PARC_MDM_MAX_SEQ 64
#define PARC_MDM_MAX_STEPS 4096                  /* timesteps of one parc_mdm_sample */
#define PARC_MDM_GRID 31                         /* the tokenizer cnn_31xy_4layer_c64_out64: 31 x 31 heights -> 64 tokens of 256 */
#define PARC_MDM_DDIM 0
#define PARC_MDM_DDPM 1
/* parc_mdm_forward variants (predict_x0 :836-852) */
#define PARC_MDM_PASS_PLAIN 0                    /* fast_forward on the cached tokens, mask and indicator */
#define PARC_MDM_PASS_GUIDED 1                   /* guidance, first pass: cached tokens and mask, the indicator forced true for the overwrite */
#define PARC_MDM_PASS_UNCOND 2                   /* guidance, second pass: indicator row 0, previous-state tokens masked, no overwrite */
typedef struct ParcMdm ParcMdm;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMdmParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t d_model, num_heads, d_hid, num_layers;
    int32_t seq_len, num_prev_states, diffusion_timesteps;
    int32_t frame_dim;                       /* 3 + 3 + 3 (B - 1) + dof_size + B: ROOT_POS, ROOT_ROT, JOINT_POS, JOINT_ROT, CONTACTS */
    int32_t target_dim;                      /* 2 (XY_DIR) */
    int32_t num_target_hidden, num_in_hidden, num_out_hidden;
    int32_t target_hidden[PARC_MDM_MAX_HIDDEN], in_hidden[PARC_MDM_MAX_HIDDEN], out_hidden[PARC_MDM_MAX_HIDDEN];
    int32_t max_batch;                       /* the largest B of parc_mdm_embed_conds / parc_mdm_sample */
    /* the weights, fp32, as one flat host buffer and num_tensors + 1 offsets (floats) into it, in this order (torch layouts):
     * conv 1..4 (weight, bias); _obs_embed (w, b); the indicator embedding [2][d]; the timestep table [timesteps][d]; the positional
     * table [tokens][d]; time_embed.0 (w, b), time_embed.2 (w, b); per layer in_proj (w, b), out_proj (w, b), linear1 (w, b),
     * linear2 (w, b), norm1 (w, b), norm2 (w, b); the linears (w, b) of the target MLP, of _in_mlp_gen_seq, of _out_mlp */
    const float *weights_host;
    const int64_t *weight_offsets_host;
    int32_t num_tensors;
    const float *mean_host, *std_host;       /* [seq_len][frame_dim] */
    /* DiffusionRates, [diffusion_timesteps] each */
    const float *sqrt_alphas_cumprod_host, *sqrt_one_minus_alphas_cumprod_host, *posterior_mean_coef1_host, *posterior_mean_coef2_host,
                *posterior_std_host;
} ParcMdmParams;
typedef struct {                             /* device arrays of one batch of conditions (MDMKeyType) */
    int32_t n;
    const float *hf;                         /* [n][31][31], clamped and divided by max_h */
    const float *target;                     /* [n][2] */
    const float *prev_state;                 /* [n][num_prev_states][frame_dim], standardised; may be null when num_prev_states is 0 */
    const int32_t *obs_flag, *target_flag, *prev_state_flag, *noise_ind;   /* [n] 0 / 1 */
} ParcMdmConds;
typedef struct {
    int32_t mode;                            /* PARC_MDM_DDIM / PARC_MDM_DDPM */
    int32_t num_steps;
    const int32_t *timesteps_host;           /* [num_steps], descending; a step at t = 0 returns the projected x_0 */
    int32_t stride;                          /* DDIM: next_t = t - stride */
    int32_t use_guidance;
    float guidance_scale;
    float *x;                                /* [n][seq_len][frame_dim] device: x_T in (unless draw), the sample out */
    const float *noise;                      /* DDPM, injected: [num_steps][n][seq_len][frame_dim] device, or NULL */
    int32_t draw;                            /* x_T (and the DDPM noise when `noise` is NULL) from Philox4x32-10 + Box-Muller keyed by */
    uint64_t seed, first_index;              /*   (seed, first_index + sample, step): independent of the batch */
    float *keep;                             /* [num_steps][n][seq_len][frame_dim] device: x after every step, or NULL */
} ParcMdmSampleArgs;
int parc_mdm_create(const ParcMdmParams *p, ParcMdm **out);
void parc_mdm_destroy(ParcMdm *h);
/* MDMTransformer.embed_conds: the condition tokens and the flags of the batch, cached in the handle.  tokens_out [n][65][d_model]
 * (64 heightfield tokens, the target token) and mask_out [n] uint64 x 3 (bit j of the key-padding mask) may be NULL.  No host sync. */
int parc_mdm_embed_conds(ParcMdm *h, const ParcMdmConds *c, float *tokens_out, uint64_t *mask_out, void *stream);
/* One pass on the cached conditions at timestep t: x [n][seq_len][frame_dim] (its first num_prev_states frames overwritten in place
 * where the pass's indicator is set), x0_out [n][seq_len][frame_dim].  No host sync. */
int parc_mdm_forward(ParcMdm *h, float *x, int32_t t, int32_t pass, float *x0_out, void *stream);
/* k_mdm_update on its own: x0 (+ guidance_scale (x0_uncond - x0) when x0_uncond is given), project_dofs, then
 * x = c0 x0 + ct x (+ cn noise); `last` != 0 stores the projected x0 instead.  x0_proj_out may be NULL. */
int parc_mdm_update(ParcMdm *h, int32_t n, const float *x0, const float *x0_uncond, float guidance_scale, float *x, int32_t last, float c0,
                    float ct, float cn, const float *noise, float *x0_proj_out, void *stream);
/* embed_conds, then num_steps x (forward, update): 1 + 2 num_steps launches, never a host sync. */
int parc_mdm_sample(ParcMdm *h, const ParcMdmConds *c, const ParcMdmSampleArgs *a, void *stream);
/* The standard-normal draws of (seed, first_index + sample, step) as out [n][seq_len][frame_dim]: step 0 is the x_T that parc_mdm_sample
 * draws, step i + 1 the DDPM noise of its step i. */
int parc_mdm_draw_noise(ParcMdm *h, int32_t n, uint64_t seed, uint64_t first_index, uint32_t step, float *out, void *stream);
/* Device time (hipEvents; waits for the last event), ms: k_mdm_cond, the k_mdm_forward launches and the k_mdm_update launches of the
 * last parc_mdm_sample (summed). */
int parc_mdm_kernel_times(ParcMdm *h, float *ms3);
/* VGPRs are the compiler's; this is what the handle chose: dynamic LDS bytes of k_mdm_forward, its grid (resident slots), scratch floats per slot. */
int parc_mdm_describe(ParcMdm *h, int64_t *out3);

/* ---- path-following motion generation: the generator's world-frame wrapper and the rollout along a path (parc_mpath_*) --
 * gen_util.gen_mdm_motion (RELATIVE_TO_ROOT) and mdm_path.generate_frames_until_end_of_path for N rows at once, each row on the terrain
 * and the path that row_path names.  A window is k_mpath_cond, parc_mdm_sample as it is, k_mpath_append; the host reads one int per
 * window (the rows not done).  A frame of the world-frame buffers is FD = 7 + 4 (B - 1) + B floats: root position 3, root rotation 4
 * (x, y, z, w), joint rotations (B - 1) x 4, contacts B.  x_T of window w of a row is the generator's draw of
 * (seed, sample index row_id * 4096 + w, step 0): it depends on the row's id, never on its place in the batch. */
#define PARC_MPATH_HEADING_AUTO 0                /* the first heading: atan2 of node 1 - node 0 */
#define PARC_MPATH_HEADING_RANDOM 1              /* uniform in [0, 2 pi), one per path */
typedef struct ParcMdmPath ParcMdmPath;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMdmPathParams) */
    ParcMdm *mdm;                            /* the generator the rollout drives; it must outlive this handle */
    float grid_dx, grid_dy;                  /* heightmap.horizontal_scale */
    int32_t num_x_neg, num_x_pos, num_y_neg, num_y_pos;   /* heightmap.local_grid: 31 x 31 points */
    float max_h;                             /* heightmap.max_h */
    float sequence_fps;
    int32_t left_foot, right_foot;           /* body ids of the done test */
    /* MDMPathSettings */
    int32_t next_node_lookahead, rewind_num_frames;
    float max_motion_length;
    /* MDMGenSettings */
    int32_t use_prev_state, use_cfg;
    float cfg_scale;
    int32_t prev_state_ind_key, target_condition_key, use_ddim, ddim_stride;
} ParcMdmPathParams;
typedef struct {                             /* device arrays that parc_mpath_conds fills, n = the scene's rows */
    float *hf;                               /* [n][31][31], minus the canonical z, clamped to +-max_h and divided by it */
    float *target;                           /* [n][2] */
    float *prev_state;                       /* [n][num_prev_states][frame_dim], standardised */
    int32_t *obs_flag, *target_flag, *prev_state_flag, *noise_ind, *done, *closest_node, *target_node;   /* [n] */
    float *canon;                            /* [n][8]: canonical xy, z, heading, heading quaternion */
} ParcMdmPathCondOut;
typedef struct {
    int32_t n;
    const float *x;                          /* [n][seq_len][frame_dim]: the sampler's result, standardised */
    const float *prev_state;                 /* [n][num_prev_states][frame_dim]: the clean previous state, standardised */
    const int32_t *noise_ind;                /* [n] */
    const float *canon;                      /* [n][8] */
    int32_t guided;                          /* the window ran under guidance: the indicator counts as false (gen_sequence) */
    int32_t lo, hi, offset;                  /* frames [lo, hi) of the window go to frames[row][offset ..] */
    float *frames;                           /* [n][max_frames][FD] */
    int32_t max_frames;
    float *prev_next;                        /* [n][num_prev_states][FD] or NULL: frames [start_frame - num_prev_states, start_frame) */
    const int32_t *done;                     /* with final_frame, or both NULL: final_frame[row] = total where done and still -1 */
    int32_t *final_frame;
    int32_t total;
} ParcMdmPathAppendArgs;
typedef struct {
    const float *prev_frames;                /* device [n][num_prev_states][FD], or NULL: blank frames, the last at node 0 */
    const float *rel_height_host;            /* [P] relative root height of the start, or NULL: drawn in [0.7, 0.9) from seed */
    const float *heading_host;               /* [P] first heading, or NULL: heading_mode */
    int32_t heading_mode;                    /* PARC_MPATH_HEADING_* */
    const float *noise;                      /* device [noise_windows][n][seq_len][frame_dim]: x_T of every window, or NULL: drawn */
    int32_t noise_windows;
    uint64_t seed;
    const int64_t *row_ids_host;             /* [n] global row ids, 0 .. 2^28 - 1, or NULL: 0 .. n - 1 */
    const int64_t *path_ids_host;            /* [P] global path ids, 0 .. 2^40 - 1, or NULL: 0 .. P - 1: the key of the drawn start */
    float *frames;                           /* out, device [n][max_frames][FD] (max_frames: parc_mpath_describe) */
    int32_t *final_frame;                    /* out, device [n]: frames at the first window that saw the row done, -1 if none */
    int32_t *done;                           /* out, device [n]: the done flags of the last window */
} ParcMdmPathRolloutArgs;
int parc_mpath_create(const ParcMdmPathParams *p, ParcMdmPath **out);
void parc_mpath_destroy(ParcMdmPath *h);
/* Host arrays, copied: terrains hf [P][X][Y] with min_points [P][2] and common dx / dy, paths [P][max_nodes][3] with counts [P] (a path
 * has 2 .. max_nodes finite nodes; path p lies on terrain p), row_path [num_rows] (num_rows <= the generator's max_batch). */
int parc_mpath_set_scene(ParcMdmPath *h, const float *hf_host, int32_t num_terrains, int32_t dim_x, int32_t dim_y, const float *min_points_host, float dx,
                         float dy, const float *paths_host, const int32_t *path_counts_host, int32_t max_nodes, const int32_t *row_path_host,
                         int32_t num_rows);
/* k_mpath_cond on its own: prev_frames device [n][num_prev_states][FD].  first != 0: the target is node 1 (the path's start);
 * blank != 0: the indicator is off (a start from blank frames); else it is on for first != 0 (given frames at the path's start, as the
 * rollout's first window) and use_prev_state otherwise.  No host sync. */
int parc_mpath_conds(ParcMdmPath *h, const float *prev_frames, int32_t first, int32_t blank, const ParcMdmPathCondOut *o, void *stream);
/* k_mpath_append on its own.  No host sync. */
int parc_mpath_append(ParcMdmPath *h, const ParcMdmPathAppendArgs *a, void *stream);
/* The whole rollout: windows x (3 + 2 steps) launches, one more for blank previous frames; one 4-byte read-back per window after the first. */
int parc_mpath_rollout(ParcMdmPath *h, const ParcMdmPathRolloutArgs *a, void *stream);
/* Device ms of the last rollout's k_mpath_cond and k_mpath_append launches (summed; waits for the last event). */
int parc_mpath_kernel_times(ParcMdmPath *h, float *ms2);
/* max_frames, max_windows, FD; then of the last rollout: windows, kernel launches, frames per row. */
int parc_mpath_describe(ParcMdmPath *h, int64_t *out6);

/* ---- rollout selection: score, filter and rank the rows of a rollout on the device (parc_msel_*) ---------------------
 * The end of mdm_path.generate_frames_until_end_of_path (mdm_path.py:386-433) and the acceptance test of parc_2_kin_gen.py:389-404.  A
 * row's motion is frames[0:final_frame] as Python slices it (-1 drops the last frame).  With slice_terrain it is scored on its own slice
 * of its terrain (terrain_util.slice_terrain_around_motion, localize=False: the root's xy bounds -+ slice_padding, rounded to grid
 * points; cells beyond the terrain repeat its edge cells), else on the whole terrain; base_z is the lowest height of that view - 10.
 * contact = w_contact x sum, pen = w_pen x sum, total = contact + pen (+ not_finished_penalty where final_frame < 0, + noise); a row is
 * valid when all three lie under their thresholds.  The rows of a path are ranked by total, ascending and stable, NaN last.  The scene,
 * the character and the layout of the frame buffer are the path handle's.  A row's results do not depend on its batch. */
#define PARC_MSEL_MAX_SLICE_DIM 1024             /* cells per side of a slice */
#define PARC_MSEL_STATUS_NONFINITE 1             /* a root position of the row's motion is not finite */
#define PARC_MSEL_STATUS_TOO_LARGE 2             /* a side of the slice exceeds PARC_MSEL_MAX_SLICE_DIM */
#define PARC_MSEL_STATUS_EMPTY 4                 /* the row's motion has no frame */
#define PARC_MSEL_RUN_LAUNCHES 4                 /* kernel launches of one parc_msel_run */
typedef struct ParcPathSelect ParcPathSelect;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcPathSelectParams) */
    ParcMdmPath *mpath;                      /* the path handle: its scene, character, max_batch and max_frames; it must outlive this handle */
    int32_t num_points;                      /* as ParcMotionTerrainParams */
    const float *points_host;                /* [num_points][3] body-local */
    const int32_t *point_body_host;          /* [num_points] */
    int32_t contact_body_id[PARC_MAX_BODIES];/* column of a frame's contacts of each body, -1 = not scored */
    float w_contact, w_pen;                  /* MDMPathSettings */
    float not_finished_penalty;              /* reference: 100 */
    float slice_padding;                     /* reference: 1.2 */
    int32_t sdf_mode;                        /* PARC_MTERR_SDF_* */
} ParcPathSelectParams;
typedef struct {
    const float *frames;                     /* device [n][frame_stride][FD], parc_mpath_rollout's layout; n = the scene's rows */
    int32_t num_frames;                      /* frames of the rollout, 1 .. min(frame_stride, the path handle's max_frames) */
    int32_t frame_stride;                    /* frames a row of the buffer holds */
    const int32_t *final_frame;              /* device [n] */
    const float *noise;                      /* device [n] added to the totals, or NULL */
    int32_t slice_terrain;
    float max_contact_loss, max_pen_loss, max_total_loss;   /* INFINITY = off */
} ParcPathSelectArgs;
typedef struct {                             /* host arrays, NULL = not copied */
    float *contact_loss, *pen_loss, *total_loss;   /* [n] weighted; total as ranked; NaN for a row with a status bit */
    int32_t *valid, *status, *num_frames;    /* [n] */
    float *slice_min_point;                  /* [n][2]: of the view the row was scored on (the terrain's without slice_terrain) */
    int32_t *slice_dims;                     /* [n][2] */
    int32_t *order;                          /* [n]: the rows of path 0 sorted, then those of path 1, ... */
    int32_t *num_valid;                      /* [P] */
} ParcPathSelectResults;
int parc_msel_create(const ParcPathSelectParams *p, ParcPathSelect **out);
void parc_msel_destroy(ParcPathSelect *h);
/* k_msel_bounds, k_msel_fk, k_msel_score, k_msel_rank on the stream; no host sync.  PARC_ERR_STATE without a scene. */
int parc_msel_run(ParcPathSelect *h, const ParcPathSelectArgs *a, void *stream);
/* The last run's results to the host (waits for the stream). */
int parc_msel_results(ParcPathSelect *h, const ParcPathSelectResults *r, void *stream);
/* The heightfields of the views of the named rows, packed one after the other (row i: dims[0] x dims[1] floats, none for a row with a
 * status bit): the sliced_hf of terrain_util.py:1613.  One launch; capacity = the floats hf_host holds. */
int parc_msel_gather(ParcPathSelect *h, const int32_t *rows_host, int32_t count, float *hf_host, int64_t capacity, void *stream);
/* Device ms of the last run: bounds, fk, score, rank, and gather (the last parc_msel_gather; 0 = none).  Waits for the events. */
int parc_msel_kernel_times(ParcPathSelect *h, float *ms5);
/* launches of the last run, max rows, max frames, PARC_MSEL_MAX_SLICE_DIM, sample points, rows of the last run. */
int parc_msel_describe(ParcPathSelect *h, int64_t *out6);

/* Hesitation-frame removal for B clips at once: the reference's medit_lib.remove_hesitation_frames
 * (util/motion_edit_lib.py:804-878), the step of stage 2 between the optimiser and compute_hf_extra_vals.  Its own handle.  The clips use
 * the optimiser's layout (ParcMotionOptClips; the heightfield arrays are validated and otherwise unused, the constraint fields ignored).
 * d(i, j) is the norm of body_pos[j] - body_pos[i] over all num_bodies x 3 numbers (FK in fp32).  Frames are visited in order: a frame i
 * that is not flagged flags every j > i with d(i, j) < hesitation_val; a flagged frame flags nothing; frame 0 is never flagged.  Runs of
 * consecutive flagged frames shorter than hesitation_min_seq_len are unflagged again; the other flagged frames are removed, and the kept
 * frames are copied as they are.  A distance that is not a number flags nothing.  Results do not depend on which other clips are in the
 * batch. */
#define PARC_MEDIT_MAX_FRAMES 4096               /* frames per clip: the flag set of a clip is one 64-bit word per lane of a wave */
#define PARC_MEDIT_FLAG_WORDS 64                 /* PARC_MEDIT_MAX_FRAMES / 64 */
typedef struct ParcMotionEdit ParcMotionEdit;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionEditParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    float hesitation_val;                    /* metres, compared in fp32 (reference default 0.15) */
    int32_t hesitation_min_seq_len;          /* >= 1 (reference default 4) */
} ParcMotionEditParams;
int parc_medit_create(const ParcMotionEditParams *p, ParcMotionEdit **out);
void parc_medit_destroy(ParcMotionEdit *h);
/* Uploads the clips (num_clips >= 1, every clip 1 .. PARC_MEDIT_MAX_FRAMES frames: PARC_ERR_INVALID names the first clip, by index, that
 * has more; nothing is truncated).  As parc_mopt_set_clips: PARC_ERR_INVALID leaves the batch loaded before in place and usable; a failure
 * after the validation leaves no batch (PARC_ERR_STATE until a parc_medit_set_clips succeeds).  The pair mask takes
 * frames x ceil(frames / 64) 64-bit words of device memory per clip. */
int parc_medit_set_clips(ParcMotionEdit *h, const ParcMotionOptClips *c);
/* One pass over the uploaded clips.  Outputs (NULL = not copied): kept_counts [num_clips]; kept_inds [F], clip c's kept source frames
 * (clip-local, ascending) from frame_off[c] on, -1 behind the first kept_counts[c]; total_kept = sum of kept_counts. */
int parc_medit_run(ParcMotionEdit *h, int32_t *kept_counts_host, int32_t *kept_inds_host, int64_t *total_kept);
/* The kept frames of the last run, clips in order: root_pos [total_kept][3], root_rot [total_kept][4], joint_rot [total_kept][B-1][4],
 * contacts [total_kept][B]; every row is a copy of its source row. */
int parc_medit_get_frames(ParcMotionEdit *h, float *root_pos_host, float *root_rot_host, float *joint_rot_host, float *contacts_host);
/* TEST entry: the pair mask of clip `clip` of the last run, [frames][ceil(frames / 64)] words: bit (j & 63) of word (j >> 6) of row i is
 * set when j > i and d(i, j) < hesitation_val. */
int parc_medit_get_pair_rows(ParcMotionEdit *h, int32_t clip, uint64_t *rows_host);
/* TEST entry: the flag words of the last run, [num_clips][PARC_MEDIT_FLAG_WORDS] each (bit j & 63 of word j >> 6 = frame j): after the
 * ordered scan, and after the run filter (either may be NULL). */
int parc_medit_get_flags(ParcMotionEdit *h, uint64_t *raw_host, uint64_t *filtered_host);
/* Device time (hipEvents) of the last run, ms: fk, pairs, scan, and gather (the last parc_medit_get_frames). */
int parc_medit_kernel_times(ParcMotionEdit *h, float *ms4);

/* Contact labelling, penetration lift and resampling of raw clips for B clips at once, each on its own terrain:
 * the reference editor's compute_hf_foot_contacts_and_correct_pen, compute_motion_terrain_hand_contacts,
 * compute_ground_plane_foot_contacts / correct_foot_ground_pen and change_motion_fps (util/motion_edit_lib.py:430-604, :752-784).  Its
 * own handle; the clips use the optimiser's layout (ParcMotionOptClips, the constraint fields ignored; the input contacts are read only by
 * keep_existing and by the resampling).  FK in fp32 on the clip's quaternions.
 * Feet: the eight corners offset +- half of a foot's first box, rotated by the body and added to its position; on the terrain a corner's
 * cell is get_grid_index (round half to even, clamped) and h its height: contact = any(z < h + contact_eps), gap = min(z - h), lift =
 * -min(0, gap of either foot).  On the ground plane: contact = any(z - ground_height - contact_eps < 0), gap = min(z - ground_height),
 * lift = ground_height - min(ground_height, z of every corner of every listed box).
 * Hands: sd = min over ALL cells of the clip's terrain of sdBox(p - centre, half) - hand_radius, each cell a column from min(hf) - 10 up
 * to its height on the centres of torch.linspace(0, (dim - 1) d, dim) + min_point; contact = sd < contact_eps.  Terrain mode only.
 * Labels, gap, lift and hand_sd come from the pose before the lift.  Results do not depend on which other clips are in the batch. */
#define PARC_MLABEL_MAX_FOOT_BOXES 8            /* box geoms of both feet together */
typedef struct ParcMotionLabel ParcMotionLabel;
typedef struct {
    uint32_t struct_size;                    /* sizeof(ParcMotionLabelParams) */
    int32_t device;
    ParcCharModel model;                     /* the tables parc_env_create takes (fk_paths unused) */
    int32_t foot_body[2];                    /* left, right: columns 0 / 1 of gap */
    int32_t hand_body[2];                    /* left, right: columns 0 / 1 of hand_sd */
    float hand_radius[2];                    /* the sphere of each hand's first geom, > 0 */
    int32_t num_foot_boxes;                  /* 2 .. PARC_MLABEL_MAX_FOOT_BOXES; every foot has at least one */
    int32_t box_foot[PARC_MLABEL_MAX_FOOT_BOXES];        /* 0 / 1: the foot of box q; the first one listed for a foot is its first geom */
    float box_offset[PARC_MLABEL_MAX_FOOT_BOXES][3];     /* in the body's frame */
    float box_half[PARC_MLABEL_MAX_FOOT_BOXES][3];       /* half extents, > 0 */
    float contact_eps;                       /* metres, compared in fp32 (reference default 0.04) */
} ParcMotionLabelParams;
int parc_mlabel_create(const ParcMotionLabelParams *p, ParcMotionLabel **out);
void parc_mlabel_destroy(ParcMotionLabel *h);
/* Uploads the clips (num_clips >= 1, every clip >= 1 frame, a terrain of fewer than 2^31 cells each).  As parc_medit_set_clips:
 * PARC_ERR_INVALID leaves the batch loaded before in place; a failure after the validation leaves no batch. */
int parc_mlabel_set_clips(ParcMotionLabel *h, const ParcMotionOptClips *c);
/* k_mlabel_feet, then k_mlabel_hands when hands != 0 and use_ground == 0.  correct_pen: the output root height is z + lift.  use_ground:
 * the plane at ground_height instead of the terrains (the hand columns are then not labelled).  keep_existing: the columns that are not
 * labelled hold the clip's own contacts instead of 0. */
int parc_mlabel_run(ParcMotionLabel *h, int32_t hands, int32_t correct_pen, int32_t use_ground, float ground_height, int32_t keep_existing);
/* The last run's root_pos [F][3] and contacts [F][num_bodies], frames in batch order. */
int parc_mlabel_get_frames(ParcMotionLabel *h, float *root_pos_host, float *contacts_host);
/* TEST entries of the last run: gap [F][2]; lift [F]; hand_sd [F][2] (+inf where the hands were not labelled). */
int parc_mlabel_get_gap(ParcMotionLabel *h, float *gap_host);
int parc_mlabel_get_lift(ParcMotionLabel *h, float *lift_host);
int parc_mlabel_get_hand_sd(ParcMotionLabel *h, float *hand_sd_host);
/* MotionLib.calc_motion_frame (LoopMode.CLAMP, anim/motion_lib.py:94-126) of the loaded clips at the caller's times: clip c's output
 * frames are out_off[c] .. out_off[c + 1] (at least one each), times_host [N] seconds, lengths_host [C] the fp32 (frames - 1) / fps > 0.
 * Root position and contacts are lerped, the rotations normalised (quat_normalize) and slerped.  Outputs [N] rows, as parc_medit_get_frames. */
int parc_mlabel_resample(ParcMotionLabel *h, const int64_t *out_off_host, const float *times_host, const float *lengths_host,
                         float *root_pos_host, float *root_rot_host, float *joint_rot_host, float *contacts_host);
/* Device time (hipEvents) of the last run and the last resample, ms: feet, hands (0 = not run), resample. */
int parc_mlabel_kernel_times(ParcMotionLabel *h, float *ms3);

#ifdef __cplusplus
}
#endif
#endif /* PARC_ENV_H */
