// parc_char.hpp — the character as the motion tools see it (parc_mopt_*, parc_mterr_*, parc_msamp_*, parc_maug_*, parc_mdm_*,
// parc_mpath_*): the kinematic tree, the sample points on its bodies, the forward kinematics over the tree and
// the small vector helpers the tools share.  No kernel lives here, and no tool's own data: a tool that needs more than the tree or the
// points derives its own struct from these (the optimiser's Model), so a change there moves no field under another tool's kernels.
//
// CharTree and CharPoints stay trivially copyable: a handle zeroes one with memset (model_zero), fills it on the host and uploads it
// with one copy (model_upload); the kernels read it from global memory through a pointer.  `pre` is the caller's message prefix.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_math.hpp"

namespace parc {

struct CharTree {                       // global memory, read with uniform indices
    int B, D;
    int parent[PARC_MAX_BODIES], jtype[PARC_MAX_BODIES], dof_idx[PARC_MAX_BODIES];
    float lt[PARC_MAX_BODIES][3], lr[PARC_MAX_BODIES][4], axis[PARC_MAX_BODIES][3];
};

struct CharPoints : CharTree {          // + the sample points, grouped by body, and the contact column of every body
    int P;
    int pt_start[PARC_MAX_BODIES], pt_count[PARC_MAX_BODIES];
    int contact_id[PARC_MAX_BODIES];
    float pts[PARC_MOPT_MAX_POINTS][3];
    int pt_body[PARC_MOPT_MAX_POINTS];
};

__device__ __forceinline__ V3 add3(V3 a, V3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 scl3(V3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 ld3(const float *p) { return mk3(p[0], p[1], p[2]); }
__device__ __forceinline__ Q4 ld4(const float *p) { return mk4(p[0], p[1], p[2], p[3]); }
__device__ __forceinline__ void st3(float *p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ void st4(float *p, Q4 q) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }
__device__ __forceinline__ void acc3(float *p, V3 v) { p[0] += v.x; p[1] += v.y; p[2] += v.z; }
__device__ __forceinline__ void acc4(float *p, Q4 q) { p[0] += q.x; p[1] += q.y; p[2] += q.z; p[3] += q.w; }
// Hamilton product written out (the adjoint products; the forward keeps parc::quat_mul's factored form)
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
    return mk4(a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
               a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z);
}

// ---- adjoints of the rotation helpers (the optimiser's and the generator loss's gradients) --------------------------------------
// d/dq of quat_rotate(q, v) = v + w t + u x t, t = 2 u x v, applied to g: gu = 2w (v x g) + t x g + 2 v x (g x u), gw = g . t
__device__ __forceinline__ Q4 rotate_vjp_q(Q4 q, V3 v, V3 g) {
    const V3 u = mk3(q.x, q.y, q.z);
    const V3 t = scl3(cross3(u, v), 2.f);
    const V3 a = scl3(cross3(v, g), 2.f * q.w), b = cross3(t, g), c = scl3(cross3(v, cross3(g, u)), 2.f);
    return mk4(a.x + b.x + c.x, a.y + b.y + c.y, a.z + b.z + c.z, dot3(g, t));
}

// quat_diff_angle(q0, q1) = angle of quat_pos(q1 (x) conj(q0)) (torch_util.py:454-462, :70-91): adjoints of q0 and q1 for dL/dangle = ga.
// Masked (|v| <= 1e-5, angle forced to 0) => zero, as autograd gives through torch.where.
__device__ __forceinline__ void diff_angle_vjp(Q4 q0, Q4 q1, float ga, Q4 &g0, Q4 &g1) {
    const Q4 dq = quat_mul(q1, quat_conj(q0));
    const float s = dq.w < 0.f ? -1.f : 1.f;
    const V3 v = mk3(s * dq.x, s * dq.y, s * dq.z);
    const float w = s * dq.w, len = norm3(v);
    if (!(len > 1e-5f) || ga == 0.f) { g0 = mk4(0.f, 0.f, 0.f, 0.f); g1 = g0; return; }
    const float r2 = len * len + w * w;
    const float kv = ga * 2.f * w / r2 / len, kw = -ga * 2.f * len / r2;
    const Q4 gdq = mk4(s * kv * v.x, s * kv * v.y, s * kv * v.z, s * kw);
    g1 = qmul(gdq, q0);
    g0 = quat_conj(qmul(quat_conj(q1), gdq));
}

// exp_map_to_quat backward (torch_util.py:426-450): q = (sin(th/2) e/|e|, cos(th/2)), th = |e| wrapped to (-pi, pi].  Masked
// |th| <= 1e-5 => 0 (the reference's backward is NaN at an exactly zero exp map: 0 here).
__device__ __forceinline__ V3 exp_map_vjp(V3 e, Q4 g) {
    const float t0 = norm3(e);
    const float th = atan2f(sinf(t0), cosf(t0));
    if (!(fabsf(th) > 1e-5f)) return mk3(0.f, 0.f, 0.f);
    const V3 n = scl3(e, 1.f / t0);
    const float s = sinf(0.5f * th), c = cosf(0.5f * th);
    const V3 gv = mk3(g.x, g.y, g.z);
    const float nd = dot3(n, gv);
    const float a = s / t0, bn = 0.5f * c * nd - a * nd - 0.5f * s * g.w;
    return mk3(a * gv.x + bn * n.x, a * gv.y + bn * n.y, a * gv.z + bn * n.z);
}

// hinge: axis_angle_to_quat(axis, d) backward
__device__ __forceinline__ float hinge_vjp(const float *axis, float d, Q4 g) {
    const V3 na = normalize3(mk3(axis[0], axis[1], axis[2]));
    return 0.5f * cosf(0.5f * d) * (na.x * g.x + na.y * g.y + na.z * g.z) - 0.5f * sinf(0.5f * d) * g.w;
}

__device__ __forceinline__ Q4 dof_rot(const CharTree &M, int j, const float *dof) {
    const int t = M.jtype[j];
    if (t == PARC_JOINT_HINGE) return axis_angle_to_quat(mk3(M.axis[j][0], M.axis[j][1], M.axis[j][2]), dof[M.dof_idx[j]]);
    if (t == PARC_JOINT_SPHERICAL) {
        const float *d = dof + M.dof_idx[j];
        return exp_map_to_quat(mk3(d[0], d[1], d[2]));
    }
    return mk4(0.f, 0.f, 0.f, 1.f);
}

// FK of one frame (kin_char_model.py:617-649) into pos / rot ([B][3], [B][4]); jrot [B][4], body 0 unused
__device__ __forceinline__ void fk_frame(const CharTree &M, V3 rp, Q4 rq, const float *jrot, float *pos, float *rot) {
    st3(pos, rp); st4(rot, rq);
    for (int j = 1; j < M.B; ++j) {
        const int p = M.parent[j];
        const Q4 pr = ld4(rot + 4 * p);
        const V3 wt = quat_rotate(pr, mk3(M.lt[j][0], M.lt[j][1], M.lt[j][2]));
        const V3 pp = ld3(pos + 3 * p);
        st3(pos + 3 * j, add3(pp, wt));
        st4(rot + 4 * j, quat_mul(pr, quat_mul(mk4(M.lr[j][0], M.lr[j][1], M.lr[j][2], M.lr[j][3]), ld4(jrot + 4 * j))));
    }
}

}  // namespace parc

// ---- host: fill and upload ---------------------------------------------------------------------------------------------------
// all of a handle's model (CharTree, CharPoints or a tool's struct derived from them) to zero bytes, before the fills below: the size
// is the caller's struct's, which the fills over the base structs cannot know
template <typename Model> static void model_zero(Model &M) { memset(&M, 0, sizeof(M)); }

// B, D and the tree of cm into M, after model_zero (the caller has checked num_bodies and dof_size against the limits)
static int model_tree(const char *pre, const ParcCharModel &cm, parc::CharTree &M) {
    M.B = cm.num_bodies; M.D = cm.dof_size;
    for (int b = 0; b < M.B; ++b) {
        M.parent[b] = cm.parent[b]; M.jtype[b] = cm.joint_type[b]; M.dof_idx[b] = cm.dof_idx[b];
        if (b > 0 && (cm.parent[b] < 0 || cm.parent[b] >= b)) return fail(PARC_ERR_INVALID, std::string(pre) + ": parents must precede their children");
        for (int k = 0; k < 3; ++k) { M.lt[b][k] = cm.local_translation[b][k]; M.axis[b][k] = cm.joint_axis[b][k]; }
        for (int k = 0; k < 4; ++k) M.lr[b][k] = cm.local_rotation[b][k];
    }
    return PARC_OK;
}

// the sample points, grouped by body (pt_start / pt_count), and the contact column of every body; after model_zero (pt_count is
// counted up from 0) and model_tree
static int model_points(const char *pre, parc::CharPoints &M, int num_points, const float *points_host, const int32_t *point_body_host,
                        const int32_t *contact_body_id) {
    M.P = num_points;
    for (int b = 0; b < M.B; ++b) {
        M.contact_id[b] = contact_body_id[b];
        if (M.contact_id[b] >= M.B) return fail(PARC_ERR_INVALID, std::string(pre) + ": contact_body_id out of range");
    }
    int prev = -1;
    for (int k = 0; k < M.P; ++k) {
        const int b = point_body_host[k];
        if (b < 0 || b >= M.B || b < prev) return fail(PARC_ERR_INVALID, std::string(pre) + ": point bodies must be in [0, B) and non-decreasing");
        if (b != prev) M.pt_start[b] = k;
        M.pt_count[b]++;
        prev = b;
        M.pt_body[k] = b;
        for (int d = 0; d < 3; ++d) M.pts[k][d] = points_host[3 * k + d];
    }
    return PARC_OK;
}

// the handle's copy of the model (CharTree, CharPoints or a tool's struct derived from them) on the current device, from `mem`
template <typename Model> static int model_upload(DeviceArena &mem, const Model &M, Model *&d_model) { return mem.alloc(d_model, 1, &M); }
