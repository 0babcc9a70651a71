// parc_env_ops.hpp — the env's kernels off the step path: the motion library's frame records (k_motion_prep), the one-thread-per-item
// operators of the C API (calc_motion_frame, dof <-> rot, FK), the recorder and the test entry point of the quaternion functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/parc_env.h"
#include "parc_common.hpp"       // MotionMeta, frame_blend
#include "parc_env_tables.hpp"   // DevTables, REC_*, joint_dof_to_rot / joint_rot_to_dof, blended_root_pos
#include "parc_math.hpp"

// ------------------------------------------------------------------------------------------------
// motion library preparation (motion_lib.py:305-327, kin_char_model.py:651-693): one thread per frame
// ------------------------------------------------------------------------------------------------
struct PrepParams {
    int F, B, J, D;
    const float *root_pos, *root_rot, *joint_rot, *contacts;
    const int *frame_motion; // [F]
    const MotionMeta *meta;
    const DevTables *tables;
    float4 *records;
};

__global__ void k_motion_prep(const PrepParams P) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= P.F) return;
    const int m = P.frame_motion[f];
    const MotionMeta meta = P.meta[m];
    const DevTables *T = P.tables;
    float4 *rec = P.records + (size_t)f * REC_F4;
    float *recf = (float *)rec;
    for (int i = 0; i < 128; ++i) recf[i] = 0.f;
    const float *rr = P.root_rot + 4 * (size_t)f;
    rec[0] = make_float4(rr[0], rr[1], rr[2], rr[3]);
    for (int j = 0; j < P.J; ++j) {
        const float *q = P.joint_rot + 4 * ((size_t)f * P.J + j);
        rec[1 + j] = make_float4(q[0], q[1], q[2], q[3]);
    }
    const float *rp = P.root_pos + 3 * (size_t)f;
    rec[REC_Q_POS] = make_float4(rp[0], rp[1], rp[2], 0.f);
    for (int b = 0; b < P.B; ++b) recf[4 * REC_Q_CONTACT + b] = P.contacts ? P.contacts[(size_t)f * P.B + b] : 0.f;
    // velocities: finite difference (f0, f0+1); the last frame repeats the previous pair
    const int local = f - meta.start;
    int f0 = f;
    if (local == meta.nframes - 1) f0 = f - 1;
    if (meta.nframes < 2) return;
    const float fps = meta.fps;
    const float dt = (float)(1.0 / (double)meta.fps);
    const float *p0 = P.root_pos + 3 * (size_t)f0, *p1 = p0 + 3;
    recf[4 * REC_Q_VEL + 0] = fps * (p1[0] - p0[0]);
    recf[4 * REC_Q_VEL + 1] = fps * (p1[1] - p0[1]);
    recf[4 * REC_Q_VEL + 2] = fps * (p1[2] - p0[2]);
    const float *r0 = P.root_rot + 4 * (size_t)f0, *r1 = r0 + 4;
    const Q4 dq = quat_mul(mk4(r1[0], r1[1], r1[2], r1[3]), quat_conj(mk4(r0[0], r0[1], r0[2], r0[3]))); // quat_diff :454
    const V3 ev = quat_to_exp_map(dq);
    recf[4 * (REC_Q_VEL + 1) + 0] = fps * ev.x;
    recf[4 * (REC_Q_VEL + 1) + 1] = fps * ev.y;
    recf[4 * (REC_Q_VEL + 1) + 2] = fps * ev.z;
    float *dv = recf + 4 * (REC_Q_VEL + 2);
    for (int j = 1; j < P.B; ++j) { // compute_dof_vel kin_char_model.py:661
        const float *a = P.joint_rot + 4 * ((size_t)f0 * P.J + j - 1), *b = a + 4 * P.J;
        const Q4 d = quat_normalize(quat_mul(quat_conj(mk4(a[0], a[1], a[2], a[3])), mk4(b[0], b[1], b[2], b[3])));
        const int ty = T->h.jtype[j];
        if (ty == PARC_JOINT_HINGE) {
            V3 x = quat_to_exp_map(d);
            x = mk3(x.x / dt, x.y / dt, x.z / dt);
            dv[T->h.dof_idx[j]] = T->h.axis[j][0] * x.x + T->h.axis[j][1] * x.y + T->h.axis[j][2] * x.z;
        } else if (ty == PARC_JOINT_SPHERICAL) {
            const V3 x = quat_to_exp_map(d);
            dv[T->h.dof_idx[j] + 0] = x.x / dt;
            dv[T->h.dof_idx[j] + 1] = x.y / dt;
            dv[T->h.dof_idx[j] + 2] = x.z / dt;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// one-thread-per-item operators (cfg-1 plumbing, reset): calc_motion_frame, dof<->rot, FK
// ------------------------------------------------------------------------------------------------
struct FrameOut { float *root_pos, *root_rot, *root_vel, *root_ang_vel, *joint_rot, *dof_vel, *contacts; };

__device__ void motion_frame_thread(const float4 *records, const MotionMeta meta, float t, int B, int J, int D, size_t o,
                                    const FrameOut &F) {
    const Blend bl = frame_blend(meta, t);
    const float4 *r0 = records + (size_t)bl.i0 * REC_F4, *r1 = records + (size_t)bl.i1 * REC_F4;
    const float b = bl.b, a = 1.0f - b;
    const V3 rp = blended_root_pos(r0, r1, b, meta, t);
    F.root_pos[3 * o] = rp.x; F.root_pos[3 * o + 1] = rp.y; F.root_pos[3 * o + 2] = rp.z;
    const Q4 rr = slerp(r0[0], r1[0], b);
    *(float4 *)(F.root_rot + 4 * o) = rr;
    for (int j = 0; j < J; ++j) *(float4 *)(F.joint_rot + 4 * (o * J + j)) = slerp(r0[1 + j], r1[1 + j], b);
    const float *v = (const float *)(r0 + REC_Q_VEL);
    if (F.root_vel) { F.root_vel[3 * o] = v[0]; F.root_vel[3 * o + 1] = v[1]; F.root_vel[3 * o + 2] = v[2]; }
    if (F.root_ang_vel) { F.root_ang_vel[3 * o] = v[4]; F.root_ang_vel[3 * o + 1] = v[5]; F.root_ang_vel[3 * o + 2] = v[6]; }
    if (F.dof_vel) for (int d = 0; d < D; ++d) F.dof_vel[o * D + d] = v[8 + d];
    if (F.contacts) {
        const float *c0 = (const float *)(r0 + REC_Q_CONTACT), *c1 = (const float *)(r1 + REC_Q_CONTACT);
        for (int k = 0; k < B; ++k) F.contacts[o * B + k] = a * c0[k] + b * c1[k];
    }
}

__global__ void k_calc_motion_frame(const float4 *records, const MotionMeta *meta, const int *ids, const float *times, int n,
                                    int B, int J, int D, FrameOut F) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    motion_frame_thread(records, meta[ids[i]], times[i], B, J, D, (size_t)i, F);
}

__global__ void k_dof_to_rot(const DevTables *T, const float *dof, float *jr, int n, int B, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int j = 1; j < B; ++j)
        *(float4 *)(jr + 4 * ((size_t)i * (B - 1) + j - 1)) = joint_dof_to_rot(T->h.jtype[j], T->h.axis[j], dof + (size_t)i * D + T->h.dof_idx[j]);
}

__global__ void k_rot_to_dof(const DevTables *T, const float *jr, float *dof, int n, int B, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int d = 0; d < D; ++d) dof[(size_t)i * D + d] = 0.f;
    for (int j = 1; j < B; ++j)
        joint_rot_to_dof(T->h.jtype[j], T->h.axis[j], *(const float4 *)(jr + 4 * ((size_t)i * (B - 1) + j - 1)), dof + (size_t)i * D + T->h.dof_idx[j]);
}

__device__ void fk_thread(const DevTables *T, int B, V3 root_pos, Q4 root_rot, const float *jr, float *bp, float *br) {
    Q4 rot[PARC_MAX_BODIES];
    V3 pos[PARC_MAX_BODIES];
    rot[0] = root_rot; pos[0] = root_pos;
    for (int j = 1; j < B; ++j) {
        const int p = T->h.parent[j];
        const V3 wt = quat_rotate(rot[p], mk3(T->h.lt[j][0], T->h.lt[j][1], T->h.lt[j][2]));
        pos[j] = mk3(pos[p].x + wt.x, pos[p].y + wt.y, pos[p].z + wt.z);
        const Q4 q = *(const float4 *)(jr + 4 * (j - 1));
        rot[j] = quat_mul(rot[p], quat_mul(mk4(T->h.lr[j][0], T->h.lr[j][1], T->h.lr[j][2], T->h.lr[j][3]), q));
    }
    for (int j = 0; j < B; ++j) {
        bp[3 * j] = pos[j].x; bp[3 * j + 1] = pos[j].y; bp[3 * j + 2] = pos[j].z;
        if (br) *(float4 *)(br + 4 * j) = rot[j];
    }
}

__global__ void k_fk(const DevTables *T, const float *root_pos, const float *root_rot, const float *jr, float *bp, float *br,
                     int n, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *rp = root_pos + 3 * (size_t)i, *rr = root_rot + 4 * (size_t)i;
    fk_thread(T, B, mk3(rp[0], rp[1], rp[2]), mk4(rr[0], rr[1], rr[2], rr[3]), jr + 4 * (size_t)i * (B - 1),
              bp + 3 * (size_t)i * B, br ? br + 4 * (size_t)i * B : nullptr);
}

// Recorder: one 128-thread block per env appends that env's row (see include/parc_env.h).
__global__ __launch_bounds__(128) void k_record(const DevTables *__restrict__ T, ParcEnvBuffers buf, int N, int B, int D, int obs_dim, float *frames,
                                                float *obs_out, int cap, int *count, unsigned char *writing, int *n_writing, int use_ref) {
    const int e = blockIdx.x, tid = threadIdx.x;
    if (e >= N || !writing[e]) return;
    const int t = count[e];
    const int W = 3 + 4 + 4 * (B - 1) + B;
    if (t < cap) {
        float *row = frames + ((size_t)t * N + e) * W;
        const float *rp = use_ref ? buf.ref_root_pos : buf.char_root_pos, *rr = use_ref ? buf.ref_root_rot : buf.char_root_rot;
        if (tid < 3) row[tid] = rp[3 * (size_t)e + tid];
        if (tid < 4) row[3 + tid] = rr[4 * (size_t)e + tid];
        if (tid >= 1 && tid < B) {
            Q4 q;
            if (use_ref) q = *(const float4 *)(buf.ref_joint_rot + 4 * ((size_t)e * (B - 1) + tid - 1));
            else q = joint_dof_to_rot(T->h.jtype[tid], T->h.axis[tid], buf.char_dof_pos + (size_t)e * D + T->h.dof_idx[tid]);
            float *o = row + 7 + 4 * (tid - 1);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        }
        if (tid < B) {
            float c;
            if (use_ref) c = buf.ref_contacts[(size_t)e * B + tid];
            else {
                const float *f = buf.contact_forces + 3 * ((size_t)e * B + tid);
                c = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) > 1e-5f ? 1.f : 0.f;
            }
            row[7 + 4 * (B - 1) + tid] = c;
        }
        if (obs_out) {
            const float *src = buf.obs + (size_t)e * obs_dim;
            float *dst = obs_out + ((size_t)t * N + e) * obs_dim;
            for (int i = tid; i < obs_dim; i += 128) dst[i] = src[i];
        }
    }
    __syncthreads();
    if (tid == 0) {
        const bool full = t >= cap;
        if (!full) count[e] = t + 1;
        if (buf.done[e] == PARC_DONE_FAIL || full) { // update_done ran before this: the row just written is the last one
            writing[e] = 0;
            atomicSub(n_writing, 1);
        }
    }
}

// ---- test entry point: the device quaternion functions, element-wise ------------------------------------------------
__global__ void k_test_quat_op(int op, const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ t, int n, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Q4 qa = (op == PARC_QOP_NORMALIZE3 || op == PARC_QOP_EXP_MAP_TO_QUAT || op == PARC_QOP_AA_TO_QUAT || op == PARC_QOP_ROTATE_2D)
                      ? mk4(a[3 * i], a[3 * i + 1], a[3 * i + 2], 0.f) : mk4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
    const V3 va = mk3(qa.x, qa.y, qa.z);
    Q4 qb = mk4(0.f, 0.f, 0.f, 1.f);
    V3 vb = mk3(0.f, 0.f, 0.f);
    if (b) {
        if (op == PARC_QOP_ROTATE) vb = mk3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
        else qb = mk4(b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]);
    }
    const float ts = t ? t[i] : 0.f;
    auto put4 = [&](Q4 q) { out[4 * i] = q.x; out[4 * i + 1] = q.y; out[4 * i + 2] = q.z; out[4 * i + 3] = q.w; };
    auto put3 = [&](V3 v) { out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z; };
    switch (op) {
    case PARC_QOP_MUL: put4(quat_mul(qa, qb)); break;
    case PARC_QOP_ROTATE: put3(quat_rotate(qa, vb)); break;
    case PARC_QOP_CONJ: put4(quat_conj(qa)); break;
    case PARC_QOP_POS: put4(quat_pos(qa)); break;
    case PARC_QOP_NORMALIZE3: put3(normalize3(va)); break;
    case PARC_QOP_TO_AXIS_ANGLE: { V3 ax; float an; quat_to_axis_angle(qa, ax, an); put4(mk4(ax.x, ax.y, ax.z, an)); break; }
    case PARC_QOP_AA_TO_QUAT: put4(axis_angle_to_quat(va, ts)); break;
    case PARC_QOP_EXP_MAP_TO_QUAT: put4(exp_map_to_quat(va)); break;
    case PARC_QOP_TO_EXP_MAP: put3(quat_to_exp_map(qa)); break;
    case PARC_QOP_DIFF_ANGLE: out[i] = quat_diff_angle(qa, qb); break;
    case PARC_QOP_NORMALIZE: put4(quat_normalize(qa)); break;
    case PARC_QOP_TO_TAN_NORM: { float tn[6]; quat_to_tan_norm(qa, tn); for (int c = 0; c < 6; ++c) out[6 * i + c] = tn[c]; break; }
    case PARC_QOP_SLERP: put4(slerp(qa, qb, ts)); break;
    case PARC_QOP_HEADING: out[i] = calc_heading(qa); break;
    case PARC_QOP_HEADING_QUAT_INV: put4(heading_quat_inv(calc_heading(qa))); break;
    case PARC_QOP_DIFF: put4(quat_mul(qb, quat_conj(qa))); break; // torch_util.py:454 quat_diff(q0, q1) = q1 (x) conj(q0)
    case PARC_QOP_SLERP_RR: put4(slerp_rr(qa, qb, ts)); break; // the observation kernel's reduced-range variant
    case PARC_QOP_ROTATE_2D: { // torch_util.py:651, as the ray loop of k_env_post evaluates it
        const float ch = cosf(ts), sh = sinf(ts);
        out[2 * i] = qa.x * ch - qa.y * sh; out[2 * i + 1] = qa.x * sh + qa.y * ch; break;
    }
    default: break;
    }
}
