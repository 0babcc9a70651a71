// parc_mdm_loss.hpp — the motion generator's training loss on gfx950 (parc_mloss_*, include/parc_env.h).
//
// The reference (motion_generator/mdm.py:573-692, MDM.motion_difference) evaluates thirteen weighted terms between a true window and the
// window the denoiser predicted through a per-body Python FK loop under autograd.  Here one launch of k_mloss gives, for N windows of T
// frames, the weighted per-window value of every term and the derivative of each window's sum of terms with respect to the STANDARDISED
// prediction (through unstandardise, exp_map_to_quat, joint_dof_to_rot and FK).
//
// Mapping: one workgroup per window, one lane per frame (frames beyond the block size in a strided loop), as k_mopt_grad maps a clip.
//   pass 1  unstandardise; dof_rot / exp_map_to_quat; FK of the prediction and of the truth; the per-frame sums of the eight frame terms
//   pass 2  the per-row sums of the four velocity terms (row r = frames r, r + 1; the neighbour's FK is another lane's, read after a barrier)
//   reduce  lane k sums term k over the frames in frame order, forms the term and d term / d sum (pseudo_huber needs the whole sum
//           before it can seed an adjoint: 1 / (2 sqrt(S + n c2)))
//   pass 3  the adjoints of every term into the frame's body position / rotation adjoints, adjoint FK in reverse body order, the dof /
//           exp-map backward, times the feature's std
// A window's frames, FK and adjoints live in a per-window slice of the handle's workspace in global memory (T x B x 36 floats + the
// features; at most a few hundred KB for a batch, L2-resident), so T and B are bounded by nothing but PARC_MAX_BODIES, and the kernel's
// arrays are indexed by body in memory, not in registers: no scratch.  No float atomics; every reduction runs in a fixed order inside
// the window's own block, so a window's result is bit-identical alone or in any batch, and a NaN window poisons only itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_math.hpp"
#include "parc_char.hpp"
#include "parc_tool_handle.hpp"

namespace mloss {
using namespace parc;

constexpr int NT = PARC_MLOSS_NUM_TERMS;
constexpr int THREADS = 64;
enum { T_VEL_ROOT_POS = 0, T_VEL_ROOT_ROT, T_VEL_JOINT_ROT, T_ROOT_POS, T_ROOT_ROT, T_JOINT_ROT, T_CONTACT, T_BODY_POS, T_FK_POS, T_FK_ROT,
       T_CONSIST, T_FK_VEL, T_TARGET };
constexpr float HUBER_C = 0.03f, HUBER_C2 = 0.0009f;   // mdm.py:103-109

struct Model : CharTree {               // the character (parc_char.hpp) + what is fixed at create
    float w[NT];
    float inv_dt;                       // sequence_fps
    float target_eps;
    int nprev, use_pos, use_target, huber;
};

struct Args {                           // one call: device pointers, row-major
    int N, T;
    const float *pred, *mean, *std;     // [N][T][D], [T][D], [T][D]
    const float *root_pos, *root_rot, *joint_rot, *contacts;   // [N][T][3], [N][T][4] xyzw, [N][T][B-1][4], [N][T][B]
    const float *target_dir;            // [N][2]
    float *terms, *grad;                // [N][NT], [N][T][D]
};

struct Work {                           // per window: [T][...]; each frame's slice is written by the frame's own lane
    float *f;                           // [N][T][D] the unstandardised prediction
    float *ppos, *prot, *pjr;           // prediction: body positions, body rotations, joint rotations (body-indexed, body 0 unused)
    float *tpos, *trot, *tjr;           // truth
    float *gpos, *grot;                 // adjoints of ppos / prot
    float *part;                        // [N][T][NT] per-frame (rows: per-row) sums
};

// quat_to_exp_map_grad_friendly (torch_util.py:94-114, :379-383): axis = v / (|v| + 1e-5) of quat_pos(q), masked by |v| > 1e-5
__device__ __forceinline__ V3 exp_map_gf(Q4 qin) {
    const Q4 q = quat_pos(qin);
    const float len = norm3(mk3(q.x, q.y, q.z));
    if (!(len > 1e-5f)) return (len == len) ? mk3(0.f, 0.f, 0.f) : mk3(len, len, len);
    const float ang = 2.0f * atan2f(len, q.w), d = len + 1e-5f;
    return mk3(ang * (q.x / d), ang * (q.y / d), ang * (q.z / d));
}

// its adjoint: e = angle(len, w) v / (len + eps); masked => 0, as autograd gives through torch.where
__device__ __forceinline__ Q4 exp_map_gf_vjp(Q4 qin, V3 ge) {
    const float s = qin.w < 0.f ? -1.f : 1.f;
    const V3 v = mk3(s * qin.x, s * qin.y, s * qin.z);
    const float w = s * qin.w, len = norm3(v);
    if (!(len > 1e-5f)) return mk4(0.f, 0.f, 0.f, 0.f);
    const float ang = 2.0f * atan2f(len, w), d = len + 1e-5f, r2 = len * len + w * w;
    const float vg = dot3(v, ge);
    const float a = ang / d;
    const float b = vg * ((2.f * w / r2) / d - ang / (d * d)) / len;
    const float gw = vg / d * (-2.f * len / r2);
    return mk4(s * (a * ge.x + b * v.x), s * (a * ge.y + b * v.y), s * (a * ge.z + b * v.z), s * gw);
}

// dq = q1 (x) conj(q0) (torch_util.py:454-456): the adjoints of q0 and q1 from dq's
__device__ __forceinline__ void quat_diff_vjp(Q4 q0, Q4 q1, Q4 gdq, Q4 &g0, Q4 &g1) {
    g1 = qmul(gdq, q0);
    g0 = quat_conj(qmul(quat_conj(q1), gdq));
}

__device__ __forceinline__ float sq3(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ Q4 add4(Q4 a, Q4 b) { return mk4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the angular-velocity difference of one rotation stream over row (a, b): (exp_map_gf(diff(true)) - exp_map_gf(diff(pred))) * inv_dt
__device__ __forceinline__ V3 ang_vel_err(Q4 ta, Q4 tb, Q4 pa, Q4 pb, float inv_dt) {
    const V3 et = exp_map_gf(quat_mul(tb, quat_conj(ta))), ep = exp_map_gf(quat_mul(pb, quat_conj(pa)));
    return sub3(scl3(et, inv_dt), scl3(ep, inv_dt));
}

// d (c |err|^2) / d pa, pb of ang_vel_err: err = ..., - exp_map_gf(pb (x) conj(pa)) * inv_dt
__device__ __forceinline__ void ang_vel_vjp(Q4 pa, Q4 pb, V3 err, float c, float inv_dt, Q4 &ga, Q4 &gb) {
    const V3 ge = scl3(err, -2.f * c * inv_dt);
    quat_diff_vjp(pa, pb, exp_map_gf_vjp(quat_mul(pb, quat_conj(pa)), ge), ga, gb);
}

__global__ void __launch_bounds__(THREADS) k_mloss(const Model *Mp, Args A, Work W) {
    __shared__ float s_coef[NT];        // d term / d (its sum of squares); the target term: d term / d (its dot product)
    const Model &M = *Mp;
    const int B = M.B, J = B - 1, T = A.T, D = 6 + 3 * J + M.D + B;
    const long long n = blockIdx.x;
    const int o_jp = 6, o_dof = 6 + 3 * J, o_con = 6 + 3 * J + M.D;
    const float inv_dt = M.inv_dt;
    const long long fb = n * T;         // the window's first frame in every [N][T][...] array
    float *part = W.part + fb * NT;

    // ---- pass 1: frames ----------------------------------------------------------------------------------------------------------
    for (int t = threadIdx.x; t < T; t += THREADS) {
        const long long ft = fb + t;
        float *f = W.f + ft * D;
        const float *x = A.pred + ft * D, *mu = A.mean + (long long)t * D, *sd = A.std + (long long)t * D;
        for (int k = 0; k < D; ++k) f[k] = x[k] * sd[k] + mu[k];
        float *ppos = W.ppos + ft * B * 3, *prot = W.prot + ft * B * 4, *pjr = W.pjr + ft * B * 4;
        float *tpos = W.tpos + ft * B * 3, *trot = W.trot + ft * B * 4, *tjr = W.tjr + ft * B * 4;
        st4(pjr, mk4(0.f, 0.f, 0.f, 1.f)); st4(tjr, mk4(0.f, 0.f, 0.f, 1.f));
        for (int j = 1; j < B; ++j) {
            st4(pjr + 4 * j, dof_rot(M, j, f + o_dof));
            st4(tjr + 4 * j, ld4(A.joint_rot + (ft * J + j - 1) * 4));
        }
        const V3 rp = ld3(f), trp = ld3(A.root_pos + 3 * ft);
        const Q4 rq = exp_map_to_quat(ld3(f + 3)), trq = ld4(A.root_rot + 4 * ft);
        fk_frame(M, rp, rq, pjr, ppos, prot);
        fk_frame(M, trp, trq, tjr, tpos, trot);
        float s_jr = 0.f, s_c = 0.f, s_bp = 0.f, s_fp = 0.f, s_fr = 0.f, s_cs = 0.f;
        for (int b = 0; b < B; ++b) {
            const V3 pp = ld3(ppos + 3 * b), tp = ld3(tpos + 3 * b);
            s_fp += sq3(sub3(tp, pp));
            const float a = quat_diff_angle(ld4(trot + 4 * b), ld4(prot + 4 * b));
            s_fr += a * a;
            const float dc = A.contacts[ft * B + b] - f[o_con + b];
            s_c += dc * dc;
            if (b > 0) {
                const V3 jp = ld3(f + o_jp + 3 * (b - 1));
                s_bp += sq3(sub3(tp, jp));
                s_cs += sq3(sub3(pp, jp));
                const float ja = quat_diff_angle(ld4(tjr + 4 * b), ld4(pjr + 4 * b));
                s_jr += ja * ja;
            }
        }
        const float ra = quat_diff_angle(trq, rq);
        float *p = part + t * NT;
        p[T_ROOT_POS] = sq3(sub3(trp, rp)); p[T_ROOT_ROT] = ra * ra; p[T_JOINT_ROT] = s_jr; p[T_CONTACT] = s_c; p[T_BODY_POS] = s_bp;
        p[T_FK_POS] = s_fp; p[T_FK_ROT] = s_fr; p[T_CONSIST] = s_cs;
        p[T_TARGET] = 0.f;
    }
    __syncthreads();
    // ---- pass 2: velocity rows (row t = frames t, t + 1; the last frame holds an empty row) -----------------------------------------------
    for (int t = threadIdx.x; t < T; t += THREADS) {
        float *p = part + t * NT;
        float s_rp = 0.f, s_rr = 0.f, s_jr = 0.f, s_fv = 0.f;
        if (t + 1 < T) {
            const long long fa = fb + t, fc = fa + 1;
            const float *ppa = W.ppos + fa * B * 3, *ppb = W.ppos + fc * B * 3, *tpa = W.tpos + fa * B * 3, *tpb = W.tpos + fc * B * 3;
            for (int b = 0; b < B; ++b) {
                const V3 vt = scl3(sub3(ld3(tpb + 3 * b), ld3(tpa + 3 * b)), inv_dt), vp = scl3(sub3(ld3(ppb + 3 * b), ld3(ppa + 3 * b)), inv_dt);
                const float e = sq3(sub3(vt, vp));
                s_fv += e;
                if (b == 0) s_rp = e;   // body 0 is the root: root_pos is its position
                else s_jr += sq3(ang_vel_err(ld4(W.tjr + (fa * B + b) * 4), ld4(W.tjr + (fc * B + b) * 4), ld4(W.pjr + (fa * B + b) * 4),
                                             ld4(W.pjr + (fc * B + b) * 4), inv_dt));
            }
            s_rr = sq3(ang_vel_err(ld4(W.trot + fa * B * 4), ld4(W.trot + fc * B * 4), ld4(W.prot + fa * B * 4), ld4(W.prot + fc * B * 4), inv_dt));
        }
        p[T_VEL_ROOT_POS] = s_rp; p[T_VEL_ROOT_ROT] = s_rr; p[T_VEL_JOINT_ROT] = s_jr; p[T_FK_VEL] = s_fv;
    }
    __syncthreads();
    // ---- reduce: lane k owns term k -------------------------------------------------------------------------------------------------
    if (threadIdx.x < NT) {
        const int k = threadIdx.x;
        float term = 0.f, coef = 0.f;
        const bool fk_term = k == T_FK_POS || k == T_FK_ROT || k == T_CONSIST || k == T_FK_VEL;
        if (k == T_TARGET) {
            if (M.use_target) {         // mdm.py:679-688
                const float *td = A.target_dir + 2 * n;
                const float *pl = W.ppos + (fb + T - 1) * B * 3, *pr = W.ppos + (fb + M.nprev - 1) * B * 3;
                const float dot = -td[0] * (pl[0] - pr[0]) + -td[1] * (pl[1] - pr[1]);
                term = (dot < -M.target_eps ? -M.target_eps : dot) * M.w[k];
                coef = dot >= -M.target_eps ? M.w[k] : 0.f;   // clamp(min): no gradient where it clamps
            }
        } else if (!(fk_term && !M.use_pos)) {
            float S = 0.f;
            for (int t = 0; t < T; ++t) S += part[t * NT + k];
            const int rows = (k == T_VEL_ROOT_POS || k == T_VEL_ROOT_ROT || k == T_VEL_JOINT_ROT || k == T_FK_VEL) ? T - 1 : T;
            const int per = (k == T_VEL_ROOT_POS || k == T_VEL_ROOT_ROT || k == T_ROOT_POS) ? 3 : (k == T_ROOT_ROT) ? 1 : (k == T_VEL_JOINT_ROT ||
                            k == T_BODY_POS || k == T_CONSIST) ? 3 * J : (k == T_JOINT_ROT) ? J : (k == T_CONTACT || k == T_FK_ROT) ? B : 3 * B;
            if (M.huber) {              // sqrt(sum((x - y)^2 + c2)) - c
                const float r = sqrtf(S + (float)(rows * per) * HUBER_C2);
                term = M.w[k] * (r - HUBER_C);
                coef = M.w[k] * 0.5f / r;
            } else {
                term = M.w[k] * S;
                coef = M.w[k];
            }
        }
        A.terms[n * NT + k] = term;
        s_coef[k] = coef;
    }
    __syncthreads();
    // ---- pass 3: adjoints ----------------------------------------------------------------------------------------------------------
    float c[NT];
    for (int k = 0; k < NT; ++k) c[k] = s_coef[k];
    for (int t = threadIdx.x; t < T; t += THREADS) {
        const long long ft = fb + t;
        const float *f = W.f + ft * D, *sd = A.std + (long long)t * D;
        float *g = A.grad + ft * D;
        const float *ppos = W.ppos + ft * B * 3, *prot = W.prot + ft * B * 4, *pjr = W.pjr + ft * B * 4;
        const float *tpos = W.tpos + ft * B * 3, *trot = W.trot + ft * B * 4, *tjr = W.tjr + ft * B * 4;
        float *gpos = W.gpos + ft * B * 3, *grot = W.grot + ft * B * 4;
        // the terms on body positions and rotations; the joint-position features
        for (int b = 0; b < B; ++b) {
            const V3 pp = ld3(ppos + 3 * b), tp = ld3(tpos + 3 * b);
            V3 gp = scl3(sub3(pp, tp), 2.f * c[T_FK_POS]);
            for (int side = 0; side < 2; ++side) {                 // row t - 1 (this frame is its second) and row t (its first)
                const int r = t - 1 + side;
                if (r < 0 || r + 1 >= T) continue;
                const long long fa = fb + r, fc = fa + 1;
                const V3 vt = scl3(sub3(ld3(W.tpos + (fc * B + b) * 3), ld3(W.tpos + (fa * B + b) * 3)), inv_dt);
                const V3 vp = scl3(sub3(ld3(W.ppos + (fc * B + b) * 3), ld3(W.ppos + (fa * B + b) * 3)), inv_dt);
                const float k = (side == 0 ? -2.f : 2.f) * inv_dt * (c[T_FK_VEL] + (b == 0 ? c[T_VEL_ROOT_POS] : 0.f));
                gp = add3(gp, scl3(sub3(vt, vp), k));
            }
            Q4 g0, g1;
            const Q4 tq = ld4(trot + 4 * b), pq = ld4(prot + 4 * b);
            diff_angle_vjp(tq, pq, 2.f * c[T_FK_ROT] * quat_diff_angle(tq, pq), g0, g1);
            if (b > 0) {
                const V3 jp = ld3(f + o_jp + 3 * (b - 1));
                const V3 dc = scl3(sub3(pp, jp), 2.f * c[T_CONSIST]);
                gp = add3(gp, dc);
                const V3 gj = sub3(scl3(sub3(jp, tp), 2.f * c[T_BODY_POS]), dc);
                float *o = g + o_jp + 3 * (b - 1);
                const float *s = sd + o_jp + 3 * (b - 1);
                o[0] = gj.x * s[0]; o[1] = gj.y * s[1]; o[2] = gj.z * s[2];
            }
            g[o_con + b] = 2.f * c[T_CONTACT] * (f[o_con + b] - A.contacts[ft * B + b]) * sd[o_con + b];
            st3(gpos + 3 * b, gp);
            st4(grot + 4 * b, g1);
        }
        // the root: position, target, rotation, angular velocity
        const V3 rp = ld3(f), trp = ld3(A.root_pos + 3 * ft);
        V3 grp = scl3(sub3(rp, trp), 2.f * c[T_ROOT_POS]);
        if (c[T_TARGET] != 0.f) {
            const float *td = A.target_dir + 2 * n;
            const float k = (t == T - 1 ? -c[T_TARGET] : 0.f) + (t == M.nprev - 1 ? c[T_TARGET] : 0.f);
            grp.x += k * td[0]; grp.y += k * td[1];
        }
        const Q4 rq = ld4(prot), trq = ld4(trot);
        Q4 grq, gx;
        diff_angle_vjp(trq, rq, 2.f * c[T_ROOT_ROT] * quat_diff_angle(trq, rq), gx, grq);
        for (int side = 0; side < 2; ++side) {
            const int r = t - 1 + side;
            if (r < 0 || r + 1 >= T) continue;
            const long long fa = fb + r, fc = fa + 1;
            const Q4 ta = ld4(W.trot + fa * B * 4), tb = ld4(W.trot + fc * B * 4), pa = ld4(W.prot + fa * B * 4), pb = ld4(W.prot + fc * B * 4);
            Q4 ga, gb;
            ang_vel_vjp(pa, pb, ang_vel_err(ta, tb, pa, pb, inv_dt), c[T_VEL_ROOT_ROT], inv_dt, ga, gb);
            grq = add4(grq, side == 0 ? gb : ga);
        }
        // adjoint FK (reverse body order) + the joint rotation terms + the dof backward
        for (int j = B - 1; j >= 1; --j) {
            const int p = M.parent[j];
            const V3 gpj = ld3(gpos + 3 * j);
            const Q4 gqj = ld4(grot + 4 * j), pr = ld4(prot + 4 * p), lr = mk4(M.lr[j][0], M.lr[j][1], M.lr[j][2], M.lr[j][3]);
            const Q4 jq = ld4(pjr + 4 * j), tq = ld4(tjr + 4 * j);
            acc3(gpos + 3 * p, gpj);
            acc4(grot + 4 * p, rotate_vjp_q(pr, mk3(M.lt[j][0], M.lt[j][1], M.lt[j][2]), gpj));
            acc4(grot + 4 * p, qmul(gqj, quat_conj(quat_mul(lr, jq))));
            Q4 gj = qmul(quat_conj(lr), qmul(quat_conj(pr), gqj));
            Q4 g0, g1;
            diff_angle_vjp(tq, jq, 2.f * c[T_JOINT_ROT] * quat_diff_angle(tq, jq), g0, g1);
            gj = add4(gj, g1);
            for (int side = 0; side < 2; ++side) {
                const int r = t - 1 + side;
                if (r < 0 || r + 1 >= T) continue;
                const long long fa = fb + r, fc = fa + 1;
                const Q4 ta = ld4(W.tjr + (fa * B + j) * 4), tb = ld4(W.tjr + (fc * B + j) * 4);
                const Q4 pa = ld4(W.pjr + (fa * B + j) * 4), pb = ld4(W.pjr + (fc * B + j) * 4);
                Q4 ga, gb;
                ang_vel_vjp(pa, pb, ang_vel_err(ta, tb, pa, pb, inv_dt), c[T_VEL_JOINT_ROT], inv_dt, ga, gb);
                gj = add4(gj, side == 0 ? gb : ga);
            }
            const int jt = M.jtype[j], di = M.dof_idx[j];
            float *o = g + o_dof + di;
            const float *s = sd + o_dof + di, *d = f + o_dof + di;
            if (jt == PARC_JOINT_HINGE) o[0] = hinge_vjp(M.axis[j], d[0], gj) * s[0];
            else if (jt == PARC_JOINT_SPHERICAL) {
                const V3 ge = exp_map_vjp(ld3(d), gj);
                o[0] = ge.x * s[0]; o[1] = ge.y * s[1]; o[2] = ge.z * s[2];
            }
        }
        grp = add3(grp, ld3(gpos));
        const V3 ge = exp_map_vjp(ld3(f + 3), add4(grq, ld4(grot)));
        g[0] = grp.x * sd[0]; g[1] = grp.y * sd[1]; g[2] = grp.z * sd[2];
        g[3] = ge.x * sd[3]; g[4] = ge.y * sd[4]; g[5] = ge.z * sd[5];
    }
}

}  // namespace mloss

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
struct ParcMotionLoss : tool::CharHandle<mloss::Model, DeviceEvents<2>> {   // mem: d_model
    DeviceArena work_mem;                // the workspace, grown to the largest N x T seen
    mloss::Work W{};
    long long work_frames = 0;
    bool ran = false;
};

extern "C" void parc_mloss_destroy(ParcMotionLoss *h) { tool::destroy(h); }

extern "C" int parc_mloss_create(const ParcMotionLossParams *p, ParcMotionLoss **out) {
    PARC_TRY(tool::create_args("mloss", "ParcMotionLossParams", p, out, 2, true));
    const ParcCharModel &cm = p->model;
    if (!(p->sequence_fps > 0.f)) return fail(PARC_ERR_INVALID, "mloss: sequence_fps must be > 0");
    if (p->num_prev_states < 1) return fail(PARC_ERR_INVALID, "mloss: num_prev_states must be >= 1");
    if (p->loss_fn != PARC_MLOSS_SQUARED_L2 && p->loss_fn != PARC_MLOSS_PSEUDO_HUBER)
        return fail(PARC_ERR_INVALID, "mloss: loss_fn must be PARC_MLOSS_SQUARED_L2 or PARC_MLOSS_PSEUDO_HUBER");
    mloss::Model M;
    PARC_TRY(tool::char_tree("mloss", cm, M));
    int used = 0;                         // the dofs must tile [0, dof_size): every feature column then has one writer
    PARC_TRY(tool::char_dofs("mloss", cm, used));
    if (used != cm.dof_size) return fail(PARC_ERR_INVALID, "mloss: the joints' dofs do not add up to dof_size");
    for (int t = 0; t < mloss::NT; ++t) M.w[t] = p->weights[t];
    M.inv_dt = p->sequence_fps; M.target_eps = p->target_dir_len_eps; M.nprev = p->num_prev_states;
    M.use_pos = p->use_pos_loss != 0; M.use_target = p->use_target_loss != 0; M.huber = p->loss_fn == PARC_MLOSS_PSEUDO_HUBER;
    return tool::create("mloss", p->device, M, out);
}

extern "C" int parc_mloss_eval(ParcMotionLoss *h, const ParcMotionLossArgs *a, void *stream) {
    if (!h || !a) return fail(PARC_ERR_INVALID, "mloss: null argument");
    if (a->n < 1) return fail(PARC_ERR_INVALID, "mloss: n must be >= 1");
    if (a->num_frames < 2) return fail(PARC_ERR_INVALID, "mloss: num_frames must be >= 2 (one velocity row)");
    if (h->host_model.nprev > a->num_frames) return fail(PARC_ERR_INVALID, "mloss: num_prev_states exceeds num_frames");
    if (!a->pred || !a->mean || !a->std || !a->root_pos || !a->root_rot || !a->joint_rot || !a->contacts || !a->terms || !a->grad)
        return fail(PARC_ERR_INVALID, "mloss: null array");
    if (h->host_model.use_target && !a->target_dir) return fail(PARC_ERR_INVALID, "mloss: use_target_loss needs target_dir");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int B = h->host_model.B, D = 6 + 3 * (B - 1) + h->host_model.D + B;
    const long long F = (long long)a->n * a->num_frames;
    if (F > h->work_frames) {             // the kernels in flight may still read the old workspace
        HIPCHK(hipStreamSynchronize(st));
        DeviceArena mem;
        mloss::Work W{};
        PARC_TRY(mem.alloc(W.f, F * D));
        PARC_TRY(mem.alloc(W.ppos, 3 * F * B)); PARC_TRY(mem.alloc(W.prot, 4 * F * B)); PARC_TRY(mem.alloc(W.pjr, 4 * F * B));
        PARC_TRY(mem.alloc(W.tpos, 3 * F * B)); PARC_TRY(mem.alloc(W.trot, 4 * F * B)); PARC_TRY(mem.alloc(W.tjr, 4 * F * B));
        PARC_TRY(mem.alloc(W.gpos, 3 * F * B)); PARC_TRY(mem.alloc(W.grot, 4 * F * B));
        PARC_TRY(mem.alloc(W.part, F * mloss::NT));
        h->work_mem.swap(mem);
        h->W = W; h->work_frames = F;
    }
    mloss::Args A;
    A.N = a->n; A.T = a->num_frames;
    A.pred = a->pred; A.mean = a->mean; A.std = a->std;
    A.root_pos = a->root_pos; A.root_rot = a->root_rot; A.joint_rot = a->joint_rot; A.contacts = a->contacts;
    A.target_dir = a->target_dir; A.terms = a->terms; A.grad = a->grad;
    HIPCHK(hipEventRecord(h->ev[0], st));
    PARC_TRY(tool::launch(mloss::k_mloss, dim3((unsigned)a->n), dim3(mloss::THREADS), 0, st, h->d_model, A, h->W));
    HIPCHK(hipEventRecord(h->ev[1], st));
    h->ran = true;
    return PARC_OK;
}

extern "C" int parc_mloss_kernel_times(ParcMotionLoss *h, float *ms1) {
    if (!h || !ms1) return fail(PARC_ERR_INVALID, "mloss: null argument");
    const tool::Span spans[] = {{h->ran, 0, 1}};
    return tool::span_times("mloss: nothing evaluated yet", h->device, h->ev, spans, ms1);
}
