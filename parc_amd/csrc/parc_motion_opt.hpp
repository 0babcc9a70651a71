// parc_motion_opt.hpp — the kinematic motion optimiser on gfx950 (parc_mopt_*, include/parc_env.h).
//
// The reference (motion_optimization.py) evaluates motion_terrain_contact_loss_localized (:426-656) for ONE clip with autograd and
// steps torch.optim.Adam.  Here all clips of a batch go through one sequence of short launches per iteration:
//   k_mopt_fk      lane per frame: dof_to_rot, exp_map_to_quat, FK; the frame's heightfield patch bounds (:510-529)
//   k_mopt_patch   lane per clip:  the patch size = max over the clip's frames (:529-531)
//   k_mopt_points  block per frame, lane per sample point: world point, brute-force SDF over the frame's patch (ground and inverted
//                  boxes in one scan), penetration / contact / foot-constraint terms and their adjoints, reduced per body in a fixed
//                  order into a position and a quaternion adjoint per body
//   k_mopt_grad    lane per frame: root / joint rotation terms, smoothness, sliding, jerk and hand constraints (recomputed from the
//                  neighbouring frames' FK, so no frame writes another frame's memory), adjoint FK, dof / exp-map backward
//   k_mopt_reduce  lane per (clip, term): the per-frame partial sums, in frame order
//   k_mopt_adam    lane per parameter: torch.optim.Adam (single-tensor path, fp32)
// No float atomics, no reduction whose order depends on the batch: a clip's result is bit-identical alone or in any batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_math.hpp"
#include "parc_char.hpp"
#include "parc_grid.hpp"
#include "parc_clip_batch.hpp"
#include "parc_tool_handle.hpp"

namespace mopt {
using namespace parc;

constexpr int NT = PARC_MOPT_NUM_TERMS;
constexpr int MAXP = PARC_MOPT_MAX_POINTS;
constexpr int MAXB = PARC_MAX_BODIES;
constexpr int PT_THREADS = 256;
enum { T_ROOT_POS = 0, T_ROOT_ROT, T_JOINT_ROT, T_SMOOTH, T_PEN, T_CONTACT, T_SLIDING, T_BODYCONS, T_JERK };

struct Model : CharPoints {             // the character (parc_char.hpp) + what the loss terms read; global memory, uniform indices
    int NP;
    int g0type[MAXB];
    float g0off[MAXB][3], g0rad[MAXB];
    float w[NT];
    float max_jerk;                     // already scaled by (1/30)^3
};

struct Clips : FrameClips {             // the batch (parc_clip_batch.hpp) + the source FK and the constraints
    const long long *cons_off;
    float *src_pos, *src_rot;           // source FK [F][B][3], [F][B][4]
    const int *cons_body, *cons_range; float *cons_point;
};

struct Work {                           // per-frame workspace, each frame owned by one lane / block
    float *params, *grad, *m, *v;       // [F][NP]
    float *pos, *rot, *jrot;            // [F][B][3], [F][B][4], [F][B][4] (body 0 unused)
    float *gpos, *grot;                 // [F][B][3], [F][B][4]
    long long *gbox;                    // [F][4] grid min x, y, max x, y
    int *patch;                         // [C][2]
    float *fterms;                      // [F][NT]
    float *terms;                       // [C][NT]
};

// the gradient of sdBox (parc_grid.hpp's sd_box; geom_util.py:124-145) as autograd computes it (sign(p) through abs, the clamp masks
// q >= 0 / max(q) <= 0, the first maximal component for max(dim=-1), 0 for a zero norm)
__device__ __forceinline__ V3 sd_box_grad(V3 p, V3 h) {
    const float qx = fabsf(p.x) - h.x, qy = fabsf(p.y) - h.y, qz = fabsf(p.z) - h.z;
    const float px = fmaxf(qx, 0.f), py = fmaxf(qy, 0.f), pz = fmaxf(qz, 0.f);
    const float n = sqrtf(px * px + py * py + pz * pz);
    V3 g = mk3(0.f, 0.f, 0.f);
    if (n > 0.f) g = mk3(qx >= 0.f ? px / n : 0.f, qy >= 0.f ? py / n : 0.f, qz >= 0.f ? pz / n : 0.f);
    const float m = fmaxf(qx, fmaxf(qy, qz));
    if (m <= 0.f) {
        if (qx == m) g.x += 1.f; else if (qy == m) g.y += 1.f; else g.z += 1.f;
    }
    const float sx = p.x > 0.f ? 1.f : (p.x < 0.f ? -1.f : 0.f), sy = p.y > 0.f ? 1.f : (p.y < 0.f ? -1.f : 0.f),
                sz = p.z > 0.f ? 1.f : (p.z < 0.f ? -1.f : 0.f);
    return mk3(sx * g.x, sy * g.y, sz * g.z);
}

// points_hf_sdf over the sx x sy boxes of a patch whose first cell is (x0, y0) (terrain_util.py:1736-1793): min over the boxes in the
// reference's (x-major) order, the first minimum kept.  Ground boxes span [base_z, hf]; with `air` the inverted boxes ([hf, 10]) are
// scanned in the same loop.  Returns the minima and d min / d point at the argmin boxes.
struct SdfOut { float ground, air; V3 g_ground, g_air; };
__device__ __forceinline__ SdfOut patch_sdf(V3 x, const float *hf, int Y, int x0, int y0, int sx, int sy, float pmx, float pmy, float dx,
                                            float dy, float base_z, bool air) {
    const float hx = dx / 2.f, hy = dy / 2.f;
    float bg = INFINITY, ba = INFINITY;
    int ig = 0, ia = 0;
    for (int i = 0; i < sx; ++i) {
        const float cx = (float)i * dx + pmx;
        const float *row = hf + (long long)(x0 + i) * Y + y0;
        for (int j = 0; j < sy; ++j) {
            const float cy = (float)j * dy + pmy;
            const float h = row[j];
            const float rx = x.x - cx, ry = x.y - cy;
            const float sg = sd_box(mk3(rx, ry, x.z - (h + base_z) / 2.f), mk3(hx, hy, (h - base_z) / 2.f));
            if (sg < bg) { bg = sg; ig = i * sy + j; }
            if (air) {
                const float sa = sd_box(mk3(rx, ry, x.z - (h + 10.f) / 2.f), mk3(hx, hy, (10.f - h) / 2.f));
                if (sa < ba) { ba = sa; ia = i * sy + j; }
            }
        }
    }
    SdfOut o;
    o.ground = bg; o.air = ba;
    {
        const int i = ig / sy, j = ig % sy;
        const float h = hf[(long long)(x0 + i) * Y + y0 + j];
        o.g_ground = sd_box_grad(mk3(x.x - ((float)i * dx + pmx), x.y - ((float)j * dy + pmy), x.z - (h + base_z) / 2.f),
                                 mk3(hx, hy, (h - base_z) / 2.f));
    }
    o.g_air = mk3(0.f, 0.f, 0.f);
    if (air) {
        const int i = ia / sy, j = ia % sy;
        const float h = hf[(long long)(x0 + i) * Y + y0 + j];
        o.g_air = sd_box_grad(mk3(x.x - ((float)i * dx + pmx), x.y - ((float)j * dy + pmy), x.z - (h + 10.f) / 2.f),
                              mk3(hx, hy, (10.f - h) / 2.f));
    }
    return o;
}

// ---- setup: FK of the source frames and the initial iterate (motion_optimization.py:744-758) -----------------------------------------
__global__ void k_mopt_source(const Model *Mp, Clips K, Work W) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const Model &M = *Mp;
    const int B = M.B, NP = M.NP;
    float *par = W.params + f * NP;
    const V3 rp = ld3(K.src_root_pos + 3 * f);
    const Q4 rq = ld4(K.src_root_rot + 4 * f);
    st3(par, rp);
    st3(par + 3, quat_to_exp_map(rq));
    for (int d = 0; d < M.D; ++d) par[6 + d] = 0.f;
    float *jr = W.jrot + f * B * 4;                          // the source joint rotations, body-indexed
    st4(jr, mk4(0.f, 0.f, 0.f, 1.f));
    for (int j = 1; j < B; ++j) {
        const Q4 q = ld4(K.src_jrot + (f * (B - 1) + j - 1) * 4);
        st4(jr + 4 * j, q);
        const int t = M.jtype[j];
        float *d = par + 6 + M.dof_idx[j];
        if (t == PARC_JOINT_HINGE) {                          // Joint.rot_to_dof kin_char_model.py:83-105
            V3 ax; float ang;
            quat_to_axis_angle(q, ax, ang);
            if (M.axis[j][0] * ax.x + M.axis[j][1] * ax.y + M.axis[j][2] * ax.z < 0.f) ang = ang * -1.f;
            d[0] = ang;
        } else if (t == PARC_JOINT_SPHERICAL) {
            st3(d, quat_to_exp_map(q));
        }
    }
    fk_frame(M, rp, rq, jr, K.src_pos + f * B * 3, K.src_rot + f * B * 4);
    for (int k = 0; k < NP; ++k) { W.m[f * NP + k] = 0.f; W.v[f * NP + k] = 0.f; }
}

// ---- per iteration ------------------------------------------------------------------------------------------------------------
__global__ void k_mopt_fk(const Model *Mp, Clips K, Work W) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const Model &M = *Mp;
    const int B = M.B;
    const float *par = W.params + f * M.NP;
    float *jr = W.jrot + f * B * 4, *pos = W.pos + f * B * 3, *rot = W.rot + f * B * 4;
    st4(jr, mk4(0.f, 0.f, 0.f, 1.f));
    for (int j = 1; j < B; ++j) st4(jr + 4 * j, dof_rot(M, j, par + 6));
    fk_frame(M, ld3(par), exp_map_to_quat(ld3(par + 3)), jr, pos, rot);
    // per-frame patch bounds (motion_optimization.py:510-527): xy box of the points +- 2 cells, floor / ceil, clamped to the grid
    const int c = K.frame_clip[f];
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    bool nan = false;
    for (int k = 0; k < M.P; ++k) {
        const int b = M.pt_body[k];
        const V3 x = add3(quat_rotate(ld4(rot + 4 * b), mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2])), ld3(pos + 3 * b));
        nan |= (x.x != x.x) || (x.y != x.y);
        mnx = fminf(mnx, x.x); mny = fminf(mny, x.y); mxx = fmaxf(mxx, x.x); mxy = fmaxf(mxy, x.y);
    }
    if (nan) { mnx = mny = mxx = mxy = NAN; }                 // torch.min / max propagate NaN
    const float *g = K.hf_geom + 4 * c;
    const float padx = g[2] * 2.f, pady = g[3] * 2.f, ix = 1.f / g[2], iy = 1.f / g[3];
    long long gx0 = to_i64(floorf((mnx - padx - g[0]) * ix)), gy0 = to_i64(floorf((mny - pady - g[1]) * iy));
    long long gx1 = to_i64(ceilf((mxx + padx - g[0]) * ix)), gy1 = to_i64(ceilf((mxy + pady - g[1]) * iy));
    gx0 = gx0 > 0 ? gx0 : 0; gy0 = gy0 > 0 ? gy0 : 0;
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1];
    gx1 = gx1 < X - 1 ? gx1 : X - 1; gy1 = gy1 < Y - 1 ? gy1 : Y - 1;
    long long *gb = W.gbox + 4 * f;
    gb[0] = gx0; gb[1] = gy0; gb[2] = gx1; gb[3] = gy1;
}

__global__ void k_mopt_patch(Clips K, Work W) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.C) return;
    long long sx = 1, sy = 1;                                // patch = max(max_f size, 1), then min(., dims)
    for (long long f = K.frame_off[c]; f < K.frame_off[c + 1]; ++f) {
        const long long *gb = W.gbox + 4 * f;
        const long long a = gb[2] - gb[0] + 1, b = gb[3] - gb[1] + 1;
        sx = a > sx ? a : sx; sy = b > sy ? b : sy;
    }
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1];
    W.patch[2 * c] = (int)(sx < X ? sx : X);
    W.patch[2 * c + 1] = (int)(sy < Y ? sy : Y);
}

// block per frame.  LDS: per point the penetration / foot-constraint adjoint, the clamped ground SDF and its gradient.
__global__ void __launch_bounds__(PT_THREADS) k_mopt_points(const Model *Mp, Clips K, Work W) {
    __shared__ float s_g[MAXP][3], s_cg[MAXP][3], s_c[MAXP], s_craw[MAXP], s_pen[MAXP], s_bc[MAXP];
    __shared__ float s_body[MAXB][3];
    const long long f = blockIdx.x;
    const Model &M = *Mp;
    const int B = M.B, tid = threadIdx.x;
    const int c = K.frame_clip[f];
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1];
    const int sx = W.patch[2 * c], sy = W.patch[2 * c + 1];
    const long long *gb = W.gbox + 4 * f;
    long long x0 = gb[0] < X - sx ? gb[0] : X - sx, y0 = gb[1] < Y - sy ? gb[1] : Y - sy;   // :533-535
    x0 = x0 > 0 ? x0 : 0; y0 = y0 > 0 ? y0 : 0;
    const float *g = K.hf_geom + 4 * c;
    const float pmx = g[0] + (float)x0 * g[2], pmy = g[1] + (float)y0 * g[3];
    const float *hf = K.hf + K.hf_off[c];
    const float *pos = W.pos + f * B * 3, *rot = W.rot + f * B * 4;
    const bool contact_on = M.w[T_CONTACT] != 0.f;
    const long long f_local = f - K.frame_off[c];
    const long long cb = K.cons_off[c], ce = K.cons_off[c + 1];
    for (int k = tid; k < M.P; k += PT_THREADS) {
        const int b = M.pt_body[k];
        const V3 x = add3(quat_rotate(ld4(rot + 4 * b), mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2])), ld3(pos + 3 * b));
        const SdfOut s = patch_sdf(x, hf, (int)Y, (int)x0, (int)y0, sx, sy, pmx, pmy, g[2], g[3], -10.f, true);
        // penetration: -clamp(-air_min, max=0) = air_min where air_min >= 0
        V3 gx = mk3(0.f, 0.f, 0.f);
        float pen = 0.f;
        if (s.air >= 0.f) { pen = s.air; gx = scl3(s.g_air, M.w[T_PEN]); }
        if (!(s.air == s.air)) pen = s.air;
        // foot constraints: sdSphere(cp, x, R) of the body's first 18 points, clamped at 0 (:598-602)
        float bc = 0.f;
        if (M.g0type[b] == 0 && k - M.pt_start[b] < 18) {
            for (long long q = cb; q < ce; ++q) {
                if (K.cons_body[q] != b || f_local < K.cons_range[2 * q] || f_local > K.cons_range[2 * q + 1]) continue;
                const V3 d = sub3(ld3(K.cons_point + 3 * q), x);
                const float n = norm3(d), v = n - M.g0rad[b];
                if (v >= 0.f) {
                    bc += v;
                    if (n > 0.f) gx = add3(gx, scl3(d, -M.w[T_BODYCONS] / n));
                } else if (!(v == v)) {
                    bc += v;
                }
            }
        }
        st3(s_g[k], gx);
        s_pen[k] = pen; s_bc[k] = bc;
        s_craw[k] = s.ground;
        s_c[k] = (s.ground == s.ground) ? fmaxf(s.ground, 0.f) : s.ground;
        st3(s_cg[k], s.g_ground);
    }
    __syncthreads();
    if (tid < B) {
        const int b = tid, k0 = M.pt_start[b], n = M.pt_count[b];
        const Q4 q = ld4(rot + 4 * b);
        float pen = 0.f, bc = 0.f, con = 0.f;
        int am = -1;
        const int cid = M.contact_id[b];
        if (contact_on && cid >= 0 && n > 0) {                // min over the body's points, first index kept (NaN wins like torch.min)
            float best = INFINITY;
            am = k0;
            for (int k = k0; k < k0 + n; ++k) {
                const float v = s_c[k];
                if (v < best || (!(v == v) && best == best)) { best = v; am = k; }
            }
            const float ct = K.contacts[f * B + cid];
            con = best * ct;
            if (!(s_craw[am] >= 0.f)) {
                am = -1;                                      // the clamp's mask at the chosen point
            } else {
                const float s = M.w[T_CONTACT] * ct;
                s_cg[am][0] *= s; s_cg[am][1] *= s; s_cg[am][2] *= s;
            }
        }
        V3 gp = mk3(0.f, 0.f, 0.f);
        Q4 gq = mk4(0.f, 0.f, 0.f, 0.f);
        for (int k = k0; k < k0 + n; ++k) {
            pen += s_pen[k]; bc += s_bc[k];
            V3 gk = ld3(s_g[k]);
            if (k == am) gk = add3(gk, ld3(s_cg[k]));
            gp = add3(gp, gk);
            const Q4 r = rotate_vjp_q(q, mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2]), gk);
            gq = mk4(gq.x + r.x, gq.y + r.y, gq.z + r.z, gq.w + r.w);
        }
        st3(W.gpos + (f * B + b) * 3, gp);
        st4(W.grot + (f * B + b) * 4, gq);
        s_body[b][0] = pen; s_body[b][1] = con; s_body[b][2] = bc;
    }
    __syncthreads();
    if (tid == 0) {
        float pen = 0.f, con = 0.f, bc = 0.f;
        for (int b = 0; b < B; ++b) { pen += s_body[b][0]; con += s_body[b][1]; bc += s_body[b][2]; }
        float *t = W.fterms + f * NT;
        t[T_PEN] = pen; t[T_CONTACT] = con; t[T_BODYCONS] = bc;
    }
}

// sliding mask: 0 when a constraint of body b (box / sphere first geom) covers velocity row r (:606-609)
__device__ __forceinline__ float slide_mask(const Model &M, const Clips &K, long long cb, long long ce, int b, long long r) {
    if (M.g0type[b] != 0 && M.g0type[b] != 1) return 1.f;
    for (long long q = cb; q < ce; ++q)
        if (K.cons_body[q] == b && r >= K.cons_range[2 * q] && r <= K.cons_range[2 * q + 1]) return 0.f;
    return 1.f;
}

__global__ void k_mopt_grad(const Model *Mp, Clips K, Work W) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const Model &M = *Mp;
    const int B = M.B, NP = M.NP;
    const int c = K.frame_clip[f];
    const long long f0 = K.frame_off[c], n = K.frame_off[c + 1] - f0, fl = f - f0;
    const long long cb = K.cons_off[c], ce = K.cons_off[c + 1];
    const float *par = W.params + f * NP;
    float *gr = W.grad + f * NP;
    float *gpos = W.gpos + f * B * 3, *grot = W.grot + f * B * 4;
    const float *pos = W.pos, *rot = W.rot;
    float t_jr = 0.f, t_sm = 0.f, t_sl = 0.f, t_bc = 0.f, t_jk = 0.f;
    const float c_h = 0.03f, c2 = 0.0009f;
    const bool sliding_on = M.w[T_SLIDING] != 0.f;
    // smoothness + sliding: velocity rows r = fl - 1 (this frame is its second) and r = fl (its first; the row's loss is counted here)
    for (int side = 0; side < 2; ++side) {
        const long long r = fl - 1 + side;
        if (r < 0 || r + 1 >= n) continue;
        const long long fa = f0 + r, fb = fa + 1;            // row r = pos[fb] - pos[fa]
        const float sgn = side == 0 ? 1.f : -1.f;            // d row / d pos[f]
        for (int b = 0; b < B; ++b) {
            const V3 ve = sub3(sub3(ld3(pos + (fb * B + b) * 3), ld3(pos + (fa * B + b) * 3)),
                               sub3(ld3(K.src_pos + (fb * B + b) * 3), ld3(K.src_pos + (fa * B + b) * 3)));
            const Q4 qa = ld4(rot + (fa * B + b) * 4), qb = ld4(rot + (fb * B + b) * 4);
            const float rv = quat_diff_angle(qb, qa);
            const float srv = quat_diff_angle(ld4(K.src_rot + (fb * B + b) * 4), ld4(K.src_rot + (fa * B + b) * 4));
            const float re = rv - srv;
            const float vsq = ve.x * ve.x + ve.y * ve.y + ve.z * ve.z;
            if (side == 1) t_sm += vsq + re * re;
            float gre = 2.f * M.w[T_SMOOTH] * re;
            V3 gve = scl3(ve, 2.f * M.w[T_SMOOTH]);
            if (sliding_on) {                                // pseudo-Huber (:611-615)
                const float m = slide_mask(M, K, cb, ce, b, r);
                const float fc = fmaxf(fminf(K.contacts[fb * B + b], K.contacts[fa * B + b]), 0.f);
                const float sv = sqrtf(vsq * m + c2), sr = sqrtf(re * re * m + c2);
                if (side == 1) t_sl += (sv - c_h) * fc + (sr - c_h) * fc;
                gve = add3(gve, scl3(ve, M.w[T_SLIDING] * fc * m / sv));
                gre += M.w[T_SLIDING] * fc * m * re / sr;
            }
            acc3(gpos + 3 * b, scl3(gve, sgn));
            Q4 g0, g1;                                        // angle = quat_diff_angle(q0 = rot[fb], q1 = rot[fa])
            diff_angle_vjp(qb, qa, gre, g0, g1);
            acc4(grot + 4 * b, side == 0 ? g0 : g1);
        }
    }
    // jerk: windows w = fl-3 .. fl of frames w..w+3 (:619-624); the window that starts here is counted here
    for (int k = 0; k < 4; ++k) {
        const long long w = fl - k;
        if (w < 0 || w + 3 >= n) continue;
        const float coef = k == 0 ? -1.f : (k == 1 ? 3.f : (k == 2 ? -3.f : 1.f));
        const long long a = f0 + w;
        for (int b = 0; b < B; ++b) {
            const V3 p0 = ld3(pos + (a * B + b) * 3), p1 = ld3(pos + ((a + 1) * B + b) * 3), p2 = ld3(pos + ((a + 2) * B + b) * 3),
                     p3 = ld3(pos + ((a + 3) * B + b) * 3);
            const V3 v0 = sub3(p1, p0), v1 = sub3(p2, p1), v2 = sub3(p3, p2);
            const V3 jv = sub3(sub3(v2, v1), sub3(v1, v0));
            const float mag = norm3(jv), e = mag - M.max_jerk;
            if (k == 0) t_jk += (e == e) ? fmaxf(e, 0.f) : e;
            if (e >= 0.f && mag > 0.f) acc3(gpos + 3 * b, scl3(jv, coef * M.w[T_JERK] / mag));
        }
    }
    // hand constraints: |sdSphere(cp, centre, r)| over the constraint's frames (:589-596)
    for (long long q = cb; q < ce; ++q) {
        const int b = K.cons_body[q];
        if (M.g0type[b] != 1 || fl < K.cons_range[2 * q] || fl > K.cons_range[2 * q + 1]) continue;
        const Q4 qb = ld4(rot + (f * B + b) * 4);
        const V3 off = mk3(M.g0off[b][0], M.g0off[b][1], M.g0off[b][2]);
        const V3 ctr = add3(quat_rotate(qb, off), ld3(pos + (f * B + b) * 3));
        const V3 d = sub3(ld3(K.cons_point + 3 * q), ctr);
        const float nd = norm3(d), v = nd - M.g0rad[b];
        t_bc += fabsf(v);
        const float sg = v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);
        if (nd > 0.f) {
            const V3 gc = scl3(d, -M.w[T_BODYCONS] * sg / nd);
            acc3(gpos + 3 * b, gc);
            acc4(grot + 4 * b, rotate_vjp_q(qb, off, gc));
        }
    }
    // root position / rotation
    const V3 rp = ld3(par), e = ld3(par + 3), srp = ld3(K.src_root_pos + 3 * f);
    const V3 rpe = sub3(rp, srp);
    const float t_rp = rpe.x * rpe.x + rpe.y * rpe.y + rpe.z * rpe.z;
    const Q4 rq = exp_map_to_quat(e), srq = ld4(K.src_root_rot + 4 * f);
    const float ra = quat_diff_angle(rq, srq);
    const float t_rr = ra * ra;
    // adjoint FK (reverse body order) + joint rotation terms + dof backward
    const float *jr = W.jrot + f * B * 4;
    const float *rotf = rot + f * B * 4;
    for (int j = B - 1; j >= 1; --j) {
        const int p = M.parent[j];
        const V3 gpj = ld3(gpos + 3 * j);
        const Q4 gqj = ld4(grot + 4 * j), pr = ld4(rotf + 4 * p), lr = mk4(M.lr[j][0], M.lr[j][1], M.lr[j][2], M.lr[j][3]);
        const Q4 jq = ld4(jr + 4 * j);
        acc3(gpos + 3 * p, gpj);
        acc4(grot + 4 * p, rotate_vjp_q(pr, mk3(M.lt[j][0], M.lt[j][1], M.lt[j][2]), gpj));
        acc4(grot + 4 * p, qmul(gqj, quat_conj(quat_mul(lr, jq))));
        Q4 gj = qmul(quat_conj(lr), qmul(quat_conj(pr), gqj));
        const Q4 sj = ld4(K.src_jrot + (f * (B - 1) + j - 1) * 4);
        const float ja = quat_diff_angle(jq, sj);
        t_jr += ja * ja;
        Q4 g0, g1;
        diff_angle_vjp(jq, sj, 2.f * M.w[T_JOINT_ROT] * ja, g0, g1);
        gj = mk4(gj.x + g0.x, gj.y + g0.y, gj.z + g0.z, gj.w + g0.w);
        const int t = M.jtype[j], di = M.dof_idx[j];
        if (t == PARC_JOINT_HINGE) gr[6 + di] = hinge_vjp(M.axis[j], par[6 + di], gj);
        else if (t == PARC_JOINT_SPHERICAL) st3(gr + 6 + di, exp_map_vjp(ld3(par + 6 + di), gj));
    }
    Q4 g0, g1;
    diff_angle_vjp(rq, srq, 2.f * M.w[T_ROOT_ROT] * ra, g0, g1);
    const Q4 gq0 = ld4(grot);
    st3(gr, add3(scl3(rpe, 2.f * M.w[T_ROOT_POS]), ld3(gpos)));
    st3(gr + 3, exp_map_vjp(e, mk4(gq0.x + g0.x, gq0.y + g0.y, gq0.z + g0.z, gq0.w + g0.w)));
    float *tt = W.fterms + f * NT;
    tt[T_ROOT_POS] = t_rp; tt[T_ROOT_ROT] = t_rr; tt[T_JOINT_ROT] = t_jr; tt[T_SMOOTH] = t_sm;
    tt[T_SLIDING] = t_sl; tt[T_BODYCONS] += t_bc; tt[T_JERK] = t_jk;
}

__global__ void k_mopt_reduce(Clips K, Work W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K.C * NT) return;
    const int c = i / NT, t = i % NT;
    double s = 0.0;
    for (long long f = K.frame_off[c]; f < K.frame_off[c + 1]; ++f) s += (double)W.fterms[f * NT + t];
    W.terms[i] = (float)s;
}

// torch.optim.Adam, single-tensor path in fp32 (lerp with weight 0.1 < 0.5: m + w (g - m); addcmul; addcdiv as (value * m) / denom)
__global__ void k_mopt_adam(Work W, long long n, float step_size, float bc2_sqrt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = W.grad[i];
    const float m = W.m[i] + 0.1f * (g - W.m[i]);
    const float v = W.v[i] * 0.999f + 0.001f * g * g;
    W.m[i] = m; W.v[i] = v;
    const float denom = sqrtf(v) / bc2_sqrt + 1e-8f;
    W.params[i] = W.params[i] + (-step_size * m) / denom;
}

// compute_approx_body_constraints' refinement (:124-146): one SGD step of lr on sdf^2 over the clip's whole terrain, non-inverted,
// base_z = min(hf) - 10; one lane per constraint point
__global__ void k_mopt_cons_sgd(Clips K, const int *clip, float *pts, int n, float lr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = clip[i];
    const float *g = K.hf_geom + 4 * c;
    const V3 x = ld3(pts + 3 * i);
    const SdfOut s = patch_sdf(x, K.hf + K.hf_off[c], K.hf_dims[2 * c + 1], 0, 0, K.hf_dims[2 * c], K.hf_dims[2 * c + 1], g[0], g[1], g[2],
                               g[3], K.hf_min[c] - 10.f, false);
    const float k = 2.f * s.ground;
    st3(pts + 3 * i, sub3(x, scl3(scl3(s.g_ground, k), lr)));
}

}  // namespace mopt

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcMotionOpt : tool::CharHandle<mopt::Model, DeviceEvents<7>> {   // mem: d_model
    struct Batch {                        // what one parc_mopt_set_clips loads; a batch is loaded when the handle holds one
        DeviceArena mem;
        mopt::Clips K{};
        mopt::Work W{};
        long long F = 0, adam_t = 0, ncons = 0;
    };
    std::unique_ptr<Batch> batch;
    float step_size = 1e-3f;
    float kernel_ms[6] = {};
};

extern "C" void parc_mopt_destroy(ParcMotionOpt *h) { tool::destroy(h); }

extern "C" int parc_mopt_create(const ParcMotionOptParams *p, ParcMotionOpt **out) {
    PARC_TRY(tool::create_args("mopt", "ParcMotionOptParams", p, out, 1, true));
    const ParcCharModel &cm = p->model;
    if (p->num_points < 1 || p->num_points > PARC_MOPT_MAX_POINTS || !p->points_host || !p->point_body_host)
        return fail(PARC_ERR_INVALID, "mopt: num_points must be in [1, 512] with points and point bodies given");
    mopt::Model M;
    PARC_TRY(tool::char_tree("mopt", cm, M));
    M.NP = PARC_MOPT_NP(cm.dof_size);
    PARC_TRY(tool::char_dofs("mopt", cm));
    for (int b = 0; b < M.B; ++b) {
        for (int k = 0; k < 3; ++k) M.g0off[b][k] = p->geom0_offset[b][k];
        M.g0type[b] = p->geom0_type[b]; M.g0rad[b] = p->geom0_radius[b];
    }
    PARC_TRY(model_points("mopt", M, p->num_points, p->points_host, p->point_body_host, p->contact_body_id));
    for (int t = 0; t < mopt::NT; ++t) M.w[t] = p->weights[t];
    const double dt = 1.0 / 30.0;
    M.max_jerk = (float)((double)p->max_jerk * (dt * dt * dt));
    return tool::create("mopt", p->device, M, out, [&](ParcMotionOpt &h) -> int {
        h.step_size = p->step_size;
        return PARC_OK;
    });
}

// validate; release the old batch (two would double the peak of F x B workspace); build the new one in a local; install it last
extern "C" int parc_mopt_set_clips(ParcMotionOpt *h, const ParcMotionOptClips *c) {
    if (!h || !c) return fail(PARC_ERR_INVALID, "mopt: null argument");
    PARC_TRY(clip_batch_arrays("mopt", c));
    if (!c->cons_off_host) return fail(PARC_ERR_INVALID, "mopt: null clip array");
    if (c->cons_off_host[0] != 0) return fail(PARC_ERR_INVALID, "mopt: offsets must start at 0");
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("mopt", c, cb));
    const int C = cb.C, B = h->host_model.B, NP = h->host_model.NP;
    for (int i = 0; i < C; ++i)
        if (c->cons_off_host[i + 1] < c->cons_off_host[i]) return fail(PARC_ERR_INVALID, "mopt: constraint offsets decrease");
    const long long F = cb.F, ncons = c->cons_off_host[C];
    if (ncons > 0 && (!c->cons_body_host || !c->cons_range_host || !c->cons_point_host)) return fail(PARC_ERR_INVALID, "mopt: null constraint array");
    for (long long q = 0; q < ncons; ++q)
        if (c->cons_body_host[q] < 0 || c->cons_body_host[q] >= B) return fail(PARC_ERR_INVALID, "mopt: constraint body out of range");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<ParcMotionOpt::Batch> nb;
    PARC_TRY(tool::renew("mopt", h->batch, nb));
    mopt::Clips &K = nb->K;
    mopt::Work &W = nb->W;
    DeviceArena &mem = nb->mem;
    PARC_TRY(clip_batch_upload(mem, K, c, cb, B));
    PARC_TRY(mem.alloc(K.cons_off, C + 1, c->cons_off_host));
    PARC_TRY(clip_batch_upload_frames(mem, K, cb));
    PARC_TRY(mem.alloc(K.src_pos, 3 * F * B));
    PARC_TRY(mem.alloc(K.src_rot, 4 * F * B));
    PARC_TRY(mem.alloc(K.cons_body, ncons, c->cons_body_host));
    PARC_TRY(mem.alloc(K.cons_range, 2 * ncons, c->cons_range_host));
    PARC_TRY(mem.alloc(K.cons_point, 3 * ncons, c->cons_point_host));
    PARC_TRY(mem.alloc(W.params, F * NP));
    PARC_TRY(mem.alloc(W.grad, F * NP));
    PARC_TRY(mem.alloc(W.m, F * NP));
    PARC_TRY(mem.alloc(W.v, F * NP));
    PARC_TRY(mem.alloc(W.pos, 3 * F * B));
    PARC_TRY(mem.alloc(W.rot, 4 * F * B));
    PARC_TRY(mem.alloc(W.jrot, 4 * F * B));
    PARC_TRY(mem.alloc(W.gpos, 3 * F * B));
    PARC_TRY(mem.alloc(W.grot, 4 * F * B));
    PARC_TRY(mem.alloc(W.gbox, 4 * F));
    PARC_TRY(mem.alloc(W.patch, 2 * C));
    PARC_TRY(mem.alloc(W.fterms, F * mopt::NT));
    PARC_TRY(mem.alloc(W.terms, (long long)C * mopt::NT));
    nb->F = F; nb->ncons = ncons;
    PARC_TRY(tool::launch(mopt::k_mopt_source, dim3(blocks(F, 64)), dim3(64), 0, 0, h->d_model, K, W));
    HIPCHK(hipDeviceSynchronize());
    h->batch = std::move(nb);
    return PARC_OK;
}

extern "C" int parc_mopt_set_constraint_points(ParcMotionOpt *h, const float *pts) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    const long long ncons = h->batch->ncons;
    if (ncons && !pts) return fail(PARC_ERR_INVALID, "mopt: null points");
    HIPCHK(hipSetDevice(h->device));
    if (ncons) HIPCHK(hipMemcpy(h->batch->K.cons_point, pts, 3 * (size_t)ncons * sizeof(float), hipMemcpyHostToDevice));
    return PARC_OK;
}

extern "C" int parc_mopt_set_params(ParcMotionOpt *h, const float *params) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    if (!params) return fail(PARC_ERR_INVALID, "mopt: null params");
    ParcMotionOpt::Batch &b = *h->batch;
    const size_t n = (size_t)b.F * h->host_model.NP;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(b.W.params, params, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b.W.m, 0, n * sizeof(float)));
    HIPCHK(hipMemset(b.W.v, 0, n * sizeof(float)));
    b.adam_t = 0;
    return PARC_OK;
}

extern "C" int parc_mopt_get_params(ParcMotionOpt *h, float *params) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    if (!params) return fail(PARC_ERR_INVALID, "mopt: null params");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(params, h->batch->W.params, (size_t)h->batch->F * h->host_model.NP * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}

// one loss + gradient evaluation: 5 launches on the null stream; with `timed` events bracket each launch
static int mopt_eval(ParcMotionOpt *h, bool timed) {
    const ParcMotionOpt::Batch &b = *h->batch;
    const long long F = b.F;
    const int C = b.K.C;
    if (timed) HIPCHK(hipEventRecord(h->ev[0], 0));
    PARC_TRY(tool::launch(mopt::k_mopt_fk, dim3(blocks(F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W));
    if (timed) HIPCHK(hipEventRecord(h->ev[1], 0));
    PARC_TRY(tool::launch(mopt::k_mopt_patch, dim3(blocks(C, 64)), dim3(64), 0, 0, b.K, b.W));
    if (timed) HIPCHK(hipEventRecord(h->ev[2], 0));
    PARC_TRY(tool::launch(mopt::k_mopt_points, dim3((unsigned)F), dim3(mopt::PT_THREADS), 0, 0, h->d_model, b.K, b.W));
    if (timed) HIPCHK(hipEventRecord(h->ev[3], 0));
    PARC_TRY(tool::launch(mopt::k_mopt_grad, dim3(blocks(F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W));
    if (timed) HIPCHK(hipEventRecord(h->ev[4], 0));
    PARC_TRY(tool::launch(mopt::k_mopt_reduce, dim3(blocks((long long)C * mopt::NT, 64)), dim3(64), 0, 0, b.K, b.W));
    if (timed) HIPCHK(hipEventRecord(h->ev[5], 0));
    return PARC_OK;
}

extern "C" int parc_mopt_loss_and_grad(ParcMotionOpt *h, float *terms, float *grad) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    const ParcMotionOpt::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    if (int rc = mopt_eval(h, false)) return rc;
    HIPCHK(hipDeviceSynchronize());
    if (terms) HIPCHK(hipMemcpy(terms, b.W.terms, (size_t)b.K.C * mopt::NT * sizeof(float), hipMemcpyDeviceToHost));
    if (grad) HIPCHK(hipMemcpy(grad, b.W.grad, (size_t)b.F * h->host_model.NP * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_mopt_step(ParcMotionOpt *h, int32_t n_iters, float *terms) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    if (n_iters < 0) return fail(PARC_ERR_INVALID, "mopt: n_iters must be >= 0");
    ParcMotionOpt::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    const long long n = b.F * h->host_model.NP;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < n_iters; ++it) {
        if (int rc = mopt_eval(h, true)) return rc;
        b.adam_t++;
        const double bc1 = 1.0 - pow(0.9, (double)b.adam_t), bc2 = 1.0 - pow(0.999, (double)b.adam_t);
        PARC_TRY(tool::launch(mopt::k_mopt_adam, dim3(blocks(n, 256)), dim3(256), 0, 0, b.W, n, (float)((double)h->step_size / bc1),
                           (float)sqrt(bc2)));
        HIPCHK(hipEventRecord(h->ev[6], 0));
        if (terms) HIPCHK(hipMemcpy(terms + (size_t)it * b.K.C * mopt::NT, b.W.terms, (size_t)b.K.C * mopt::NT * sizeof(float),
                                    hipMemcpyDeviceToHost));
        HIPCHK(hipEventSynchronize(h->ev[6]));
        for (int k = 0; k < 6; ++k) {              // fk, patch, points, grad, reduce, adam
            float ms = 0.f;
            PARC_TRY(h->ev.elapsed(ms, k, k + 1));
            acc[k] += ms;
        }
    }
    for (int k = 0; k < 6; ++k) h->kernel_ms[k] = n_iters ? (float)(acc[k] / n_iters) : 0.f;
    return PARC_OK;
}

extern "C" int parc_mopt_kernel_times(ParcMotionOpt *h, float *ms6) {
    return tool::stored_times("mopt", h, &ParcMotionOpt::kernel_ms, ms6);
}

extern "C" int parc_mopt_get_frames(ParcMotionOpt *h, float *root_pos, float *root_rot, float *joint_rot) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    const ParcMotionOpt::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    PARC_TRY(tool::launch(mopt::k_mopt_fk, dim3(blocks(b.F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W));
    HIPCHK(hipDeviceSynchronize());
    const int B = h->host_model.B, NP = h->host_model.NP;
    std::vector<float> rot((size_t)b.F * B * 4), jr((size_t)b.F * B * 4), par((size_t)b.F * NP);
    HIPCHK(hipMemcpy(rot.data(), b.W.rot, rot.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(jr.data(), b.W.jrot, jr.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(par.data(), b.W.params, par.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (long long f = 0; f < b.F; ++f) {
        if (root_pos) for (int k = 0; k < 3; ++k) root_pos[3 * f + k] = par[f * NP + k];
        if (root_rot) for (int k = 0; k < 4; ++k) root_rot[4 * f + k] = rot[f * B * 4 + k];
        if (joint_rot) for (int j = 1; j < B; ++j) for (int k = 0; k < 4; ++k) joint_rot[(f * (B - 1) + j - 1) * 4 + k] = jr[(f * B + j) * 4 + k];
    }
    return PARC_OK;
}

extern "C" int parc_mopt_get_source_body(ParcMotionOpt *h, float *body_pos, float *body_rot) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    const ParcMotionOpt::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)b.F * h->host_model.B;
    if (body_pos) HIPCHK(hipMemcpy(body_pos, b.K.src_pos, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (body_rot) HIPCHK(hipMemcpy(body_rot, b.K.src_rot, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_mopt_build_constraints(ParcMotionOpt *h, int32_t n, const int32_t *clip, float *pts, int32_t steps, float lr) {
    PARC_TRY(tool::check_loaded("mopt", h, &ParcMotionOpt::batch));
    if (n < 0 || steps < 0 || (n > 0 && (!clip || !pts))) return fail(PARC_ERR_INVALID, "mopt: bad constraint arguments");
    if (n == 0) return PARC_OK;
    const mopt::Clips &K = h->batch->K;
    for (int i = 0; i < n; ++i) if (clip[i] < 0 || clip[i] >= K.C) return fail(PARC_ERR_INVALID, "mopt: constraint clip out of range");
    HIPCHK(hipSetDevice(h->device));
    DeviceArena tmp;                      // this call's inputs
    int *d_clip; float *d_pts;
    PARC_TRY(tmp.alloc(d_clip, n, clip));
    PARC_TRY(tmp.alloc(d_pts, 3LL * n, pts));
    for (int s = 0; s < steps; ++s) {
        PARC_TRY(tool::launch(mopt::k_mopt_cons_sgd, dim3(blocks(n, 64)), dim3(64), 0, 0, K, d_clip, d_pts, n, lr));
    }
    HIPCHK(hipMemcpy(pts, d_pts, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}
