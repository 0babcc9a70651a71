// parc_env_tables.hpp — what the env's kernel headers (parc_env_post.hpp, parc_curriculum.hpp, parc_env_ops.hpp, parc_reset.hpp,
// parc_render.hpp) and its host code (parc_env.hip) share: the frame record layout, the device tables, StepParams, the joint <-> dof
// functions, the terrain cell index, and the small device helpers that more than one kernel uses.
// The env unit's code is at global scope with the names of parc_math.hpp visible.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/parc_env.h"
#include "parc_common.hpp"    // MotionMeta, Blend
#include "parc_lanetab.hpp"   // ParcLaneEntry, ParcHrotEntry
#include "parc_math.hpp"

using namespace parc;

// ------------------------------------------------------------------------------------------------
// device-side tables
// ------------------------------------------------------------------------------------------------
#define REC_F4 32           // one frame record = 32 float4 = 512 B
#define REC_Q_POS 15         // float4 #15 = root position
#define REC_Q_CONTACT 16     // float4 #16..19 = contacts
#define REC_Q_VEL 20         // float4 #20 = root_vel, #21 = root_ang_vel, #22.. = dof_vel

struct HierTables { // joint hierarchy.  The members up to `parent` are what every wave of k_env_post stages into LDS
    float lt[16][3];
    float lr[16][4];
    int fk_paths[PARC_MAX_FK_PATHS][PARC_MAX_FK_DEPTH];
    int key_ids[8];
    int key_slot[16]; // body -> index into key_ids, or -1
    int parent[16];   // ---- not staged (read from global memory where needed) ----
    int jtype[16];
    int dof_idx[16];
    float axis[16][4];
};
#define HIER_STAGED_WORDS ((int)(offsetof(HierTables, parent) / 4))

#define TILE_MAX_CELLS 320 // the terrain tile aliases the FK scratch (80 float4)

struct DevTables { // global memory; `h` is staged into LDS, the rest is read once per env
    HierTables h;
    float tstep[8];          // control_dt * tar_obs_steps (fp32 product, mgdm_dm_util.py:232)
    float joint_err_w[16];
    float dof_err_w[PARC_MAX_DOFS];
    float contact_w[16];
    float pose_term_dist[16];
    ParcLaneEntry lane[64];  // parc_lanetab.hpp: refilled when the tile radius changes (parc_env_load_terrain)
    ParcHrotEntry hrot[64];  // parc_lanetab.hpp: the lane's item of the heading pass and its part in the contact / velocity block
};

struct StepParams {
    int N, B, J, D, K, S, R, M, T;
    int lds_wave_floats; // dynamic LDS per wave of k_env_post
    int global_obs, off_char; // read by the OBSVAR instantiations of k_env_post only
    int lr_identity;          // every joint's fixed local rotation is the identity (the humanoid): lr (x) q = q, no quaternion product in the row phase
    int obs_tar, obs_contact; // OBSVAR only: 0 = the target block (+ target contacts) / the contact blocks and the reward's contact term are off
    int obs_dim, off_dofvel, off_key, off_tar, tar_w, off_tarc, off_cc, off_hf;
    float dt_f, episode_length, min_obs_h, max_obs_h;
    float pose_w, vel_w, root_pos_w, root_vel_w, key_pos_w;
    float root_pos_term_sq, root_rot_term;
    int early_term, pose_term, track_root, track_root_h, tracking, body_pos_from_fk, never_done;
    unsigned fall_mask;   // contact_bodies != []: bit b = body b may touch the ground (0 = the fall rule is off)
    float term_h;
    // terrain
    const float *hf; int X, Y; float min_x, min_y, dx, dy; int tile_r;
    float rdx, rdy;      // correctly rounded 1/dx, 1/dy (host): the ray loop divides by multiply + one exact correction
    float tstep[8];      // control_dt * tar_obs_steps (fp32 product, mgdm_dm_util.py:232)
    // tables
    const float4 *records; const MotionMeta *meta; const float *motion_offsets; const float *env_offsets;
    const float *ray_points; const DevTables *tables;
    // curriculum hand-off
    unsigned char *ema_code;
    unsigned *stamp_out; // diagnostic builds only
    float4 *prep;        // [N][16]: slot 0 = (cos h, sin h, hinv.z, hinv.w), slots 1..B-1 = character joint quats
    ParcEnvBuffers buf;
};

// Joint.dof_to_rot kin_char_model.py:61-81
__device__ __forceinline__ Q4 joint_dof_to_rot(int type, const float *axis4, const float *dof) {
    if (type == PARC_JOINT_HINGE) return axis_angle_to_quat(mk3(axis4[0], axis4[1], axis4[2]), dof[0]);
    if (type == PARC_JOINT_SPHERICAL) return exp_map_to_quat(mk3(dof[0], dof[1], dof[2]));
    return mk4(0.f, 0.f, 0.f, 1.f);
}

// Joint.rot_to_dof kin_char_model.py:83-105
__device__ __forceinline__ void joint_rot_to_dof(int type, const float *axis4, Q4 q, float *out) {
    if (type == PARC_JOINT_HINGE) {
        V3 axis; float angle;
        quat_to_axis_angle(q, axis, angle);
        float dot = axis4[0] * axis.x + axis4[1] * axis.y + axis4[2] * axis.z;
        if (dot < 0.f) angle = angle * -1.f;
        out[0] = angle;
    } else if (type == PARC_JOINT_SPHERICAL) {
        V3 e = quat_to_exp_map(q);
        out[0] = e.x; out[1] = e.y; out[2] = e.z;
    }
}

// Same value as cell_index (IEEE division), for a divisor whose correctly rounded reciprocal rd is known: q0 = RN(x*rd),
// the residual x - d*q0 is exact in one fma, q = RN(q0 + r*rd) is the correctly rounded quotient (Markstein's
// reciprocal-with-correction division; checked exhaustively against x/d on the CPU by tests/test_host_cpu.py for the
// grid spacings in use).  3 instructions instead of the ~13 of the general sequence; used by the 441-ray loop.
__device__ __forceinline__ float cell_float_rcp(float p, float mn, float d, float rd) { // the cell index while still a float
    const float x = p - mn;
    const float q0 = x * rd;
    const float r = fmaf(-d, q0, x);
    return rintf(fmaf(r, rd, q0));
}
__device__ __forceinline__ int cell_index_rcp(float p, float mn, float d, float rd) {
    float f = cell_float_rcp(p, mn, d, rd);
    f = fminf(fmaxf(f, -1.0e9f), 1.0e9f);
    return (int)f;
}

// terrain_util.py:146-152 — unclamped nearest cell (round half to even)
__device__ __forceinline__ int cell_index(float p, float mn, float d) {
    float f = rintf((p - mn) / d);
    f = fminf(fmaxf(f, -1.0e9f), 1.0e9f);
    return (int)f;
}

// ------------------------------------------------------------------------------------------------
// device helpers that more than one kernel of the env uses
// ------------------------------------------------------------------------------------------------
// Entry i of an env list: 64-bit ids (the C API's callers), 32-bit ids (the done list of the last step), or every env in order.
__device__ __forceinline__ int list_env(const int64_t *env_ids, const int *env_ids32, int i) {
    return env_ids ? (int)env_ids[i] : (env_ids32 ? env_ids32[i] : i);
}

// Slot j of an env's prep record (StepParams::prep): slot 0 = the heading terms of the root rotation, slot j >= 1 = the quaternion of joint j
// from the env's dofs (kin_char_model.py:586; torch_util.py:502-530).  k_env_prep and k_reset_with; k_dynamics_wave has its own copy.
__device__ __forceinline__ float4 prep_record_slot(const DevTables *T, int j, const float4 &root_rot, const float *dof) {
    if (j == 0) {
        const float heading = calc_heading(root_rot);
        const Q4 hinv = heading_quat_inv(heading);
        return make_float4(cosf(heading), sinf(heading), hinv.z, hinv.w);
    }
    return joint_dof_to_rot(T->h.jtype[j], T->h.axis[j], dof + T->h.dof_idx[j]);
}

// Root position of the frame blended from records r0 and r1 with factor b (motion_lib.py:94-128): the lerp, plus the loop offset of a
// wrapping motion at time t (_calc_loop_offset :440).
__device__ __forceinline__ V3 blended_root_pos(const float4 *r0, const float4 *r1, float b, const MotionMeta &meta, float t) {
    const float a = 1.0f - b;
    const float4 A = r0[REC_Q_POS], Bv = r1[REC_Q_POS];
    float x = a * A.x + b * Bv.x, y = a * A.y + b * Bv.y, z = a * A.z + b * Bv.z;
    if (meta.loop == PARC_LOOP_WRAP) {
        const float ph = floorf(t / meta.length);
        x = x + ph * meta.dx; y = y + ph * meta.dy; z = z + ph * meta.dz;
    }
    return mk3(x, y, z);
}

// Inclusive scan over the 64 lanes of a wave, for int and for double (two 32-bit shuffles per step).
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d, 64); if (lane >= d) v += u; }
    return v;
}
__device__ __forceinline__ double shfl_up_f64(double v, int d) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_up((int)(b & 0xffffffffll), d, 64), hi = __shfl_up((int)(b >> 32), d, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_scan_incl(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double u = shfl_up_f64(v, d); if (lane >= d) v += u; }
    return v;
}

// The totals of the 16 waves of a 1024-thread block, in LDS -> the sum of the waves before wave `wv`, and of all of them.
struct WaveTotals { int woff, total; };
__device__ __forceinline__ WaveTotals wave_totals(const int (&s_tot)[16], int wv) {
    int woff = 0, total = 0;
    for (int i = 0; i < 16; ++i) { const int c = s_tot[i]; if (i < wv) woff += c; total += c; }
    return {woff, total};
}
