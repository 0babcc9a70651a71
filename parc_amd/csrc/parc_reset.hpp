// parc_reset.hpp — resets: the sampling of a reset state, k_reset_with, and the sampling CDF of a large library (k_build_cdf).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/parc_env.h"
#include "parc_common.hpp"       // MotionMeta, frame_blend, philox4
#include "parc_env_tables.hpp"   // DevTables, REC_*, joint_rot_to_dof, list_env, prep_record_slot, blended_root_pos, wave_scan_incl
#include "parc_math.hpp"

// ---- sampling of the reset state (dm_env.py:470-504), inside k_reset_with --------------------------------------------
// The Philox call index of a sampling reset is *call_dev + 1; the observation launch that follows the reset kernel bumps
// the device-side counter (so that a captured graph replays with a fresh index every time).
#define CDF_LOCAL_MAX 64
struct SampleParams {
    int enabled;                 // 0: the caller passes motion ids / terrain ids / start times / xy noise (parc_env_reset_with)
    int M, T, rand_reset, demo_mode;
    float min_w, noise_scale;
    const float *cdf_global;     // k_build_cdf's output, libraries of more than CDF_LOCAL_MAX motions
    const float *fail_rates, *motion_weights, *start_frac;
    unsigned long long seed;
    const unsigned long long *call_dev;
};

__device__ __forceinline__ void sample_reset(const SampleParams &SP, const float *cdf, const MotionMeta *meta, int e, int &mid, int &tid, float &t0,
                                             float &nx, float &ny) {
    const unsigned long long call = *SP.call_dev + 1ull;
    float u[4], v[4];
    philox4(SP.seed, call, (unsigned)e * 2u, u);
    philox4(SP.seed, call, (unsigned)e * 2u + 1u, v);
    const int M = SP.M;
    if (SP.demo_mode) mid = e % M; // dm_env.py:479-480
    else { // multinomial with replacement == inverse CDF per draw (motion_lib.py:56-60)
        const float x = u[0] * cdf[M - 1];
        int lo = 0, hi = M - 1;
        while (lo < hi) { const int md = (lo + hi) >> 1; if (cdf[md] > x) hi = md; else lo = md + 1; }
        mid = lo;
    }
    tid = min((int)(u[1] * (float)SP.T), SP.T - 1);                                       // torch.randint(high=T)
    const float len = meta[mid].length;
    t0 = SP.rand_reset ? u[2] * len : len * (SP.start_frac ? SP.start_frac[e] : 0.f);     // motion_lib.py:62-72, dm_env.py:500-504
    nx = SP.noise_scale * (v[0] * 2.0f - 1.0f);                                           // mgdm_dm_util.py:103-104
    ny = SP.noise_scale * (v[1] * 2.0f - 1.0f);
}

// ------------------------------------------------------------------------------------------------
// reset (dm_env.py:567-592): thread per reset env
// ------------------------------------------------------------------------------------------------
struct ResetParams {
    int B, J, D, T, N;
    const float4 *records; const MotionMeta *meta; const float *motion_offsets; const float *env_offsets;
    const DevTables *tables;
    float *scratch_jr;  // [N][J][4] when ref_joint_rot is not bound
    float4 *prep;       // [N][16]: the record k_env_prep would write for the reset envs (saves that launch)
    ParcEnvBuffers buf;
};

// 16 lanes per env (4 envs per wave): lane j owns quaternion / body j of the character, lane 15 the root position.  Same
// arithmetic per quantity as the one-thread-per-env form it replaces (motion_frame_thread, joint_rot_to_dof, fk_thread),
// so results are unchanged; the per-env serial chain (15 slerps + 14 exp maps + 15-body FK, ~7k instructions) becomes ~600.
__global__ __launch_bounds__(64) void k_reset_with(const ResetParams P, const int64_t *env_ids, const int *env_ids32, const int *count_dev, int k,
                                                   const int *motion_ids, const int *terrain_ids, const float *t0, const float *xy_noise,
                                                   const SampleParams SP) {
    __shared__ float s_cdf[CDF_LOCAL_MAX];
    __shared__ float4 s_q[4][16];     // [g][0] root rotation, [g][j] joint j (j >= 1)
    __shared__ float4 s_pos[4][16];   // FK: body positions
    __shared__ float4 s_rot[4][16];   // FK: body rotations
    __shared__ float s_dof[4][PARC_MAX_DOFS];
    const int g = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int i = blockIdx.x * 4 + g;
    if (count_dev) k = *count_dev;
    if ((int)blockIdx.x * 4 >= k) return; // the grid is sized for all envs, the list is usually short
    const bool live = i < k;
    const int B = P.B, J = P.J, D = P.D;
    int e = 0, mid = 0, tid = 0;
    float t = 0.f;
    Blend bl; bl.i0 = 0; bl.i1 = 0; bl.b = 0.f;
    MotionMeta meta = P.meta[0];
    float nx = 0.f, ny = 0.f; // add_noise_to_char_state (mgdm_dm_util.py:102-106): xy += scale * U(-1,1)
    if (live) e = list_env(env_ids, env_ids32, i);
    if (SP.enabled) {
        const float *cdf = SP.cdf_global;
        if (SP.M <= CDF_LOCAL_MAX) { // the wave scan of k_build_cdf for a library that fits one wave: same operations, same result
            const int lane = threadIdx.x;
            const double v = wave_scan_incl(lane < SP.M ? (double)(fmaxf(SP.fail_rates[lane], SP.min_w) * SP.motion_weights[lane]) : 0.0, lane);
            if (lane < SP.M) s_cdf[lane] = (float)(0.0 + v);
            __syncthreads();
            cdf = s_cdf;
        }
        if (live && j == 0) sample_reset(SP, cdf, P.meta, e, mid, tid, t, nx, ny); // lane 0 of the env's 16 draws, the others receive
        mid = __shfl(mid, g * 16, 64); tid = __shfl(tid, g * 16, 64); t = __shfl(t, g * 16, 64);
        nx = __shfl(nx, g * 16, 64); ny = __shfl(ny, g * 16, 64);
    } else if (live) {
        mid = motion_ids[i]; tid = terrain_ids[i]; t = t0[i];
        nx = xy_noise[2 * i]; ny = xy_noise[2 * i + 1];
    }
    if (live) {
        meta = P.meta[mid];
        bl = frame_blend(meta, t);
    }
    const float4 *r0 = P.records + (size_t)bl.i0 * REC_F4, *r1 = P.records + (size_t)bl.i1 * REC_F4;
    const float b = bl.b, a = 1.0f - b;
    float *jr_out = P.buf.ref_joint_rot ? P.buf.ref_joint_rot : P.scratch_jr;
    for (int d = j; d < D; d += 16) s_dof[g][d] = 0.f;
    // ---- reference frame at t0 -> character state (mgdm_dm_util.py:89-100); ref_* mirrors when bound
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (live) {
        if (j < B) {
            const Q4 q = slerp(r0[j], r1[j], b);
            s_q[g][j] = q;
            if (j == 0) {
                *(float4 *)(P.buf.char_root_rot + 4 * (size_t)e) = q;
                if (P.buf.ref_root_rot) *(float4 *)(P.buf.ref_root_rot + 4 * (size_t)e) = q;
            } else {
                *(float4 *)(jr_out + 4 * ((size_t)e * J + j - 1)) = q;
            }
        }
        // every lane forms the root position (the FK lanes need it too); lane 15 stores it
        const V3 rp = blended_root_pos(r0, r1, b, meta, t);
        const float *mo = P.motion_offsets + 2 * ((size_t)mid * P.T + tid);
        const float ox = mo[0] - P.env_offsets[3 * e], oy = mo[1] - P.env_offsets[3 * e + 1];
        rx = rp.x + ox; ry = rp.y + oy; rz = rp.z;
        // velocities of frame idx0 (un-interpolated) and contacts, spread over the lanes
        const float *v = (const float *)(r0 + REC_Q_VEL);
        if (j < 3) {
            P.buf.char_root_vel[3 * (size_t)e + j] = v[j];
            P.buf.char_root_ang_vel[3 * (size_t)e + j] = v[4 + j];
            if (P.buf.ref_root_vel) P.buf.ref_root_vel[3 * (size_t)e + j] = v[j];
            if (P.buf.ref_root_ang_vel) P.buf.ref_root_ang_vel[3 * (size_t)e + j] = v[4 + j];
        }
        for (int d = j; d < D; d += 16) {
            P.buf.char_dof_vel[(size_t)e * D + d] = v[8 + d];
            if (P.buf.ref_dof_vel) P.buf.ref_dof_vel[(size_t)e * D + d] = v[8 + d];
        }
        if (P.buf.ref_contacts && j < B) {
            const float *c0 = (const float *)(r0 + REC_Q_CONTACT), *c1 = (const float *)(r1 + REC_Q_CONTACT);
            P.buf.ref_contacts[(size_t)e * B + j] = a * c0[j] + b * c1[j];
        }
    }
    __syncthreads();
    if (live && j >= 1 && j < B) joint_rot_to_dof(P.tables->h.jtype[j], P.tables->h.axis[j], s_q[g][j], &s_dof[g][P.tables->h.dof_idx[j]]);
    __syncthreads();
    // the record k_env_prep forms from the NEW state (the same function: heading terms from the root rotation, character
    // joint quaternions from the stored dofs), so the observation pass that follows needs no prep launch
    if (live && j < B) P.prep[(size_t)e * 16 + j] = prep_record_slot(P.tables, j, s_q[g][0], s_dof[g]);
    float cx = rx, cy = ry;
    if (live) { cx = rx + nx; cy = ry + ny; }
    if (live) {
        for (int d = j; d < D; d += 16) {
            P.buf.char_dof_pos[(size_t)e * D + d] = s_dof[g][d];
            if (P.buf.ref_dof_pos) P.buf.ref_dof_pos[(size_t)e * D + d] = s_dof[g][d];
        }
        if (j == 15) {
            if (P.buf.ref_root_pos) { float *o = P.buf.ref_root_pos + 3 * (size_t)e; o[0] = rx; o[1] = ry; o[2] = rz; }
            float *crp = P.buf.char_root_pos + 3 * (size_t)e;
            crp[0] = cx; crp[1] = cy; crp[2] = rz;
            P.buf.motion_ids[e] = mid;
            P.buf.terrain_ids[e] = tid;
            P.buf.time_offsets[e] = t;
            P.buf.timestep[e] = 0;
            if (P.buf.time) P.buf.time[e] = 0.f;
            P.buf.done[e] = PARC_DONE_NULL;
            if (P.buf.ep_num) P.buf.ep_num[e] += 1; // ig_parkour_env.py:826-827
        }
        if (P.buf.contact_forces) for (int c = j; c < 3 * B; c += 16) P.buf.contact_forces[(size_t)e * 3 * B + c] = 0.f;
    }
    // rigid bodies: FK of the new state (PhysX would refresh them one sim step later).  Lane j walks root -> body j; each
    // body's pose is formed from its parent's exactly as fk_thread does, level by level.
    if (P.buf.char_body_pos) {
        if (live && j == 0) { s_rot[g][0] = s_q[g][0]; s_pos[g][0] = make_float4(cx, cy, rz, 0.f); }
        __syncthreads();
        int dj = 0; // depth of body j in the tree
        if (j >= 1 && j < B) for (int q = j; q != 0; q = P.tables->h.parent[q]) ++dj;
        for (int depth = 1; depth < B; ++depth) { // level by level: body j is formed once its parent is
            if (live && j >= 1 && j < B) {
                if (dj == depth) {
                    const int p = P.tables->h.parent[j];
                    const Q4 rp_ = s_rot[g][p];
                    const float4 pp = s_pos[g][p];
                    const V3 wt = quat_rotate(rp_, mk3(P.tables->h.lt[j][0], P.tables->h.lt[j][1], P.tables->h.lt[j][2]));
                    s_pos[g][j] = make_float4(pp.x + wt.x, pp.y + wt.y, pp.z + wt.z, 0.f);
                    s_rot[g][j] = quat_mul(rp_, quat_mul(mk4(P.tables->h.lr[j][0], P.tables->h.lr[j][1], P.tables->h.lr[j][2], P.tables->h.lr[j][3]), s_q[g][j]));
                }
            }
            __syncthreads();
            if (depth >= PARC_MAX_FK_DEPTH + 1) break;
        }
        if (live && j < B) {
            float *bp = P.buf.char_body_pos + 3 * ((size_t)e * B + j);
            const float4 pj = s_pos[g][j];
            bp[0] = pj.x; bp[1] = pj.y; bp[2] = pj.z;
        }
    }
}

// weights = clamp(fail_rate, min_w) * motion_weight (dm_env.py:487-490) -> inclusive CDF (one block)
// Libraries of more than CDF_LOCAL_MAX motions; smaller ones are scanned by k_reset_with itself (one launch less on the reset path).
__global__ __launch_bounds__(1024) void k_build_cdf(const float *fail_rates, const float *motion_weights, float min_w, int M, float *cdf) {
    // rows of 1024 consecutive motions (coalesced); inside a row: wave scans through shuffles, the 16 wave totals through LDS;
    // the running total carries from row to row.  Sums are formed in double, the stored value is its fp32 rounding.
    __shared__ double s_wave[16];
    __shared__ double s_carry;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0.0;
    __syncthreads();
    for (int base0 = 0; base0 < M; base0 += 16 * 1024) { // 16 rows per pass: their loads are all in flight before the first scan
        float pv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = base0 + r * 1024 + threadIdx.x;
            pv[r] = m < M ? fmaxf(fail_rates[m], min_w) * motion_weights[m] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int base = base0 + r * 1024;
            if (base >= M) break; // uniform
            const int m = base + threadIdx.x;
            const double v = wave_scan_incl((double)pv[r], lane);
            if (lane == 63) s_wave[wv] = v;
            __syncthreads();
            double off = s_carry;
            for (int q = 0; q < wv; ++q) off += s_wave[q];
            if (m < M) cdf[m] = (float)(off + v);
            __syncthreads();
            if (threadIdx.x == 1023) s_carry = off + v;
            __syncthreads();
        }
    }
}
