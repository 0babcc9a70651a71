// parc_motion_label.hpp — contact labelling, penetration lift and resampling of raw clips on gfx950 (parc_mlabel_*, include/parc_env.h;
// DESIGN.md section 8o).
//
// What the reference's editor does one clip at a time behind "Automatic Contact Labelling" (motion_edit_lib.py:430-604), for a whole batch
// of clips, each on its own terrain:
//   k_mlabel_feet      lane per frame: FK (parc_char.hpp's fk_frame) into a per-frame workspace, the eight corners of each foot's box, the
//                      cell under every corner (parc_grid.hpp's grid_index) or the ground plane, gap / contact / lift, the output root
//                      position and every contact column but the hands'
//   k_mlabel_hands     wave per frame, lanes striding over the cells of the clip's terrain, both hands per pass: the exact minimum of the
//                      cell columns' box SDF (the analyser's ground_sd on its linspace centres), a butterfly min over the wave, then
//                      hand_sd and the two hand columns.  fminf is exact, commutative and associative: the minimum over a terrain has
//                      one value whatever the order, and the order here is fixed anyway
//   k_mlabel_resample  lane per output frame: MotionLib.calc_motion_frame (CLAMP) at the host's list of times
// No atomics and no reduction whose order depends on the batch: a clip's results are bit-identical alone or in any batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
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
#include "parc_motion_terrain.hpp"   // the analyser's linspace Axis, ground_sd and clip_base_z

namespace mlabel {
using namespace parc;

constexpr int HAND_WAVES = 4;          // frames per block of k_mlabel_hands
constexpr int MAX_BOXES = PARC_MLABEL_MAX_FOOT_BOXES;

struct Model : CharTree {              // + the feet and the hands
    int foot_body[2], hand_body[2];
    float hand_radius[2];
    int num_boxes, box_foot[MAX_BOXES], first_box[2];   // first_box[k]: the first box listed for foot k, its first geom
    float box_off[MAX_BOXES][3], box_half[MAX_BOXES][3];
};

struct Cfg {                           // by value: the settings of one run
    float eps, ground_height;
    int hands, correct_pen, ground, keep_existing;   // hands: k_mlabel_hands follows; ground: the plane instead of the terrain
};

struct Work {
    float *pos, *rot;                  // [F][B][3], [F][B][4]: fk_frame's outputs
    float *gap, *hand_sd;              // [F][2]
    float *lift;                       // [F]
    float *out_root_pos, *out_contacts;   // [F][3], [F][B]
};

struct Resample {                      // device views of one parc_mlabel_resample
    long long N;
    const int *out_clip;               // [N] the clip of every output frame
    const float *times, *length;       // [N], [C]
    float *root_pos, *root_rot, *jrot, *contacts;   // [N] rows
};

// corner s (bit 0 / 1 / 2: +x / +y / +z) of box q of the body at (bp, br): get_box_points_batch, geom_util.py:82-113
__device__ __forceinline__ V3 box_corner(const Model &M, int q, int s, V3 bp, Q4 br) {
    const float lx = (s & 1 ? M.box_half[q][0] : -M.box_half[q][0]) + M.box_off[q][0];
    const float ly = (s & 2 ? M.box_half[q][1] : -M.box_half[q][1]) + M.box_off[q][1];
    const float lz = (s & 4 ? M.box_half[q][2] : -M.box_half[q][2]) + M.box_off[q][2];
    return add3(quat_rotate(br, mk3(lx, ly, lz)), bp);
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ void k_mlabel_feet(const Model *Mp, FrameClips K, Work W, Cfg G) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const Model &M = *Mp;
    const int B = M.B;
    float *pos = W.pos + f * B * 3, *rot = W.rot + f * B * 4;
    const V3 rp = ld3(K.src_root_pos + 3 * f);
    // fk_frame reads joint j's rotation at base + 4 j for j >= 1 only
    fk_frame(M, rp, ld4(K.src_root_rot + 4 * f), K.src_jrot + f * (B - 1) * 4 - 4, pos, rot);
    const int c = K.frame_clip[f];
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1];
    const float *g = K.hf_geom + 4 * c, *hf = K.hf + K.hf_off[c];
    float *ct = W.out_contacts + f * B;
    for (int b = 0; b < B; ++b) ct[b] = G.keep_existing ? K.contacts[f * B + b] : 0.f;
    float low = G.ground ? G.ground_height : 0.f;             // min(ground_height, corners) / min(0, gaps)
    for (int k = 0; k < 2; ++k) {
        const int b = M.foot_body[k];
        const V3 bp = ld3(pos + 3 * b);
        const Q4 br = ld4(rot + 4 * b);
        float gap = INFINITY;
        bool touch = false;
        for (int s = 0; s < 8; ++s) {
            const V3 x = box_corner(M, M.first_box[k], s, bp, br);
            if (G.ground) {                                   // compute_ground_plane_foot_contacts, :465: z - eps < 0 at height 0
                touch = touch || (x.z - G.ground_height) - G.eps < 0.f;
                gap = fminf(gap, x.z - G.ground_height);
            } else {                                          // compute_hf_foot_contacts_and_correct_pen, :511-520
                const float h = hf[grid_index(x.x, g[0], g[2], X) * Y + grid_index(x.y, g[1], g[3], Y)];
                touch = touch || x.z < h + G.eps;
                gap = fminf(gap, x.z - h);
            }
        }
        W.gap[2 * f + k] = gap;
        ct[b] = touch ? 1.f : 0.f;
        if (!G.ground) low = fminf(low, gap);
    }
    if (G.ground)                                             // correct_foot_ground_pen, :586-600: every box geom of the feet
        for (int q = 0; q < M.num_boxes; ++q) {
            const int b = M.foot_body[M.box_foot[q]];
            const V3 bp = ld3(pos + 3 * b);
            const Q4 br = ld4(rot + 4 * b);
            for (int s = 0; s < 8; ++s) low = fminf(low, box_corner(M, q, s, bp, br).z);
        }
    const float lift = G.ground ? G.ground_height - low : -low;
    W.lift[f] = lift;
    st3(W.out_root_pos + 3 * f, mk3(rp.x, rp.y, G.correct_pen ? rp.z + lift : rp.z));
    if (!G.hands) { W.hand_sd[2 * f] = INFINITY; W.hand_sd[2 * f + 1] = INFINITY; }
}

__global__ void __launch_bounds__(64 * HAND_WAVES) k_mlabel_hands(const Model *Mp, FrameClips K, Work W, Cfg G) {
    // the wave's frame: the same in every lane, so its clip, the terrain's geometry and the hand positions are scalar loads
    const long long f = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long long)blockIdx.x * HAND_WAVES;
    if (f >= K.F) return;
    const Model &M = *Mp;
    const int lane = threadIdx.x & 63, B = M.B;
    const int c = K.frame_clip[f];
    const int X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1], n = X * Y;   // set_clips: X Y < 2^31
    const float *g = K.hf_geom + 4 * c, *hf = K.hf + K.hf_off[c];
    const float hx = g[2] / 2.f, hy = g[3] / 2.f, base_z = mterr::clip_base_z(K, c);
    const mterr::Axis ax = mterr::make_axis(g[0], g[2], X), ay = mterr::make_axis(g[1], g[3], Y);
    const V3 p0 = ld3(W.pos + (f * B + M.hand_body[0]) * 3), p1 = ld3(W.pos + (f * B + M.hand_body[1]) * 3);
    // cell idx = i Y + j, idx = lane, lane + 64, ...: (i, j) advance by (64 / Y, 64 % Y) with one carry, no division per cell
    const int qs = 64 / Y, rs = 64 % Y;
    int i = lane / Y, j = lane % Y;
    float m0 = INFINITY, m1 = INFINITY;
    for (int idx = lane; idx < n; idx += 64) {
        const float cx = mterr::centre(ax, i), cy = mterr::centre(ay, j), h = hf[idx];
        m0 = fminf(m0, mterr::ground_sd(p0, cx, cy, hx, hy, h, base_z));
        m1 = fminf(m1, mterr::ground_sd(p1, cx, cy, hx, hy, h, base_z));
        i += qs; j += rs;
        if (j >= Y) { j -= Y; ++i; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        m0 = fminf(m0, __shfl_xor(m0, o));
        m1 = fminf(m1, __shfl_xor(m1, o));
    }
    if (lane == 0) {                                          // points_round_boxes_sdf: sdBox - radius; x - r is monotone, so min(x) - r = min(x - r)
        const float s0 = m0 - M.hand_radius[0], s1 = m1 - M.hand_radius[1];
        W.hand_sd[2 * f] = s0; W.hand_sd[2 * f + 1] = s1;
        W.out_contacts[f * B + M.hand_body[0]] = s0 < G.eps ? 1.f : 0.f;
        W.out_contacts[f * B + M.hand_body[1]] = s1 < G.eps ? 1.f : 0.f;
    }
}

// MotionLib.calc_motion_frame with LoopMode.CLAMP (motion_lib.py:94-126, :425-438, :520-530); the library normalises the rotations
// when it loads them (:164-165)
__global__ void k_mlabel_resample(ClipArrays K, Resample R, int B) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= R.N) return;
    const int c = R.out_clip[o], J = B - 1;
    const long long f0 = K.frame_off[c], T = K.frame_off[c + 1] - f0;
    float phase = R.times[o] / R.length[c];
    phase = fminf(fmaxf(phase, 0.f), 1.f);
    const float pf = phase * (float)(T - 1);
    long long i0 = (long long)pf;
    i0 = i0 < T - 1 ? i0 : T - 1;                             // phase <= 1: equal already; a NaN time stays inside the clip
    i0 = i0 > 0 ? i0 : 0;
    const long long i1 = i0 + 1 < T - 1 ? i0 + 1 : T - 1;
    const float bl = pf - (float)i0, omb = 1.0f - bl;
    const long long a = f0 + i0, b = f0 + i1;
    for (int k = 0; k < 3; ++k) R.root_pos[3 * o + k] = omb * K.src_root_pos[3 * a + k] + bl * K.src_root_pos[3 * b + k];
    st4(R.root_rot + 4 * o, slerp(quat_normalize(ld4(K.src_root_rot + 4 * a)), quat_normalize(ld4(K.src_root_rot + 4 * b)), bl));
    for (int j = 0; j < J; ++j)
        st4(R.jrot + (o * J + j) * 4,
            slerp(quat_normalize(ld4(K.src_jrot + (a * J + j) * 4)), quat_normalize(ld4(K.src_jrot + (b * J + j) * 4)), bl));
    for (int k = 0; k < B; ++k) R.contacts[o * B + k] = omb * K.contacts[a * B + k] + bl * K.contacts[b * B + k];
}

}  // namespace mlabel

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcMotionLabel : tool::CharHandle<mlabel::Model, DeviceEvents<6>> {   // mem: d_model
    struct Batch {                        // what one parc_mlabel_set_clips loads; a batch is loaded when the handle holds one
        DeviceArena mem;
        FrameClips K{};
        mlabel::Work W{};
        std::vector<long long> frame_off;
        long long F = 0;
        bool ran = false;
    };
    float eps = 0.f;
    std::unique_ptr<Batch> batch;
    float kernel_ms[3] = {};              // feet, hands, resample
};

extern "C" void parc_mlabel_destroy(ParcMotionLabel *h) { tool::destroy(h); }

extern "C" int parc_mlabel_create(const ParcMotionLabelParams *p, ParcMotionLabel **out) {
    PARC_TRY(tool::create_args("mlabel", "ParcMotionLabelParams", p, out, 1, true));
    if (!std::isfinite(p->contact_eps)) return fail(PARC_ERR_INVALID, "mlabel: contact_eps must be finite");
    mlabel::Model M;
    PARC_TRY(tool::char_tree("mlabel", p->model, M));
    for (int k = 0; k < 2; ++k) {
        if (p->foot_body[k] < 0 || p->foot_body[k] >= M.B) return fail(PARC_ERR_INVALID, "mlabel: foot_body out of range");
        if (p->hand_body[k] < 0 || p->hand_body[k] >= M.B) return fail(PARC_ERR_INVALID, "mlabel: hand_body out of range");
        if (!(p->hand_radius[k] > 0.f) || !std::isfinite(p->hand_radius[k])) return fail(PARC_ERR_INVALID, "mlabel: hand_radius must be > 0");
        M.foot_body[k] = p->foot_body[k]; M.hand_body[k] = p->hand_body[k]; M.hand_radius[k] = p->hand_radius[k];
        M.first_box[k] = -1;
    }
    if (p->num_foot_boxes < 2 || p->num_foot_boxes > mlabel::MAX_BOXES) return fail(PARC_ERR_INVALID, "mlabel: num_foot_boxes out of range");
    M.num_boxes = p->num_foot_boxes;
    for (int q = 0; q < M.num_boxes; ++q) {
        const int k = p->box_foot[q];
        if (k < 0 || k > 1) return fail(PARC_ERR_INVALID, "mlabel: box_foot must be 0 or 1");
        M.box_foot[q] = k;
        if (M.first_box[k] < 0) M.first_box[k] = q;
        for (int d = 0; d < 3; ++d) {
            if (!std::isfinite(p->box_offset[q][d]) || !(p->box_half[q][d] > 0.f) || !std::isfinite(p->box_half[q][d]))
                return fail(PARC_ERR_INVALID, "mlabel: box " + std::to_string(q) + " needs a finite offset and half extents > 0");
            M.box_off[q][d] = p->box_offset[q][d]; M.box_half[q][d] = p->box_half[q][d];
        }
    }
    if (M.first_box[0] < 0 || M.first_box[1] < 0) return fail(PARC_ERR_INVALID, "mlabel: every foot needs a box");
    return tool::create("mlabel", p->device, M, out, [&](ParcMotionLabel &h) -> int {
        h.eps = p->contact_eps;
        return PARC_OK;
    });
}

// as parc_medit_set_clips: validate; release the old batch; build the new one in a local; install it last
extern "C" int parc_mlabel_set_clips(ParcMotionLabel *h, const ParcMotionOptClips *c) {
    if (!h || !c) return fail(PARC_ERR_INVALID, "mlabel: null argument");
    PARC_TRY(clip_batch_arrays("mlabel", c));
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("mlabel", c, cb));
    const int C = cb.C, B = h->host_model.B;
    const long long F = cb.F;
    for (int i = 0; i < C; ++i)
        if (c->hf_off_host[i + 1] - c->hf_off_host[i] > 0x7fffffffLL)
            return fail(PARC_ERR_INVALID, "mlabel: clip " + std::to_string(i) + ": at most 2^31 - 1 terrain cells");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<ParcMotionLabel::Batch> nb;
    PARC_TRY(tool::renew("mlabel", h->batch, nb));
    mlabel::Work &W = nb->W;
    DeviceArena &mem = nb->mem;
    PARC_TRY(clip_batch_upload(mem, nb->K, c, cb, B));
    PARC_TRY(clip_batch_upload_frames(mem, nb->K, cb));
    PARC_TRY(mem.alloc(W.pos, 3 * F * B));
    PARC_TRY(mem.alloc(W.rot, 4 * F * B));
    PARC_TRY(mem.alloc(W.gap, 2 * F));
    PARC_TRY(mem.alloc(W.hand_sd, 2 * F));
    PARC_TRY(mem.alloc(W.lift, F));
    PARC_TRY(mem.alloc(W.out_root_pos, 3 * F));
    PARC_TRY(mem.alloc(W.out_contacts, F * B));
    nb->F = F;
    nb->frame_off.assign(c->frame_off_host, c->frame_off_host + C + 1);
    h->batch = std::move(nb);
    return PARC_OK;
}

extern "C" int parc_mlabel_run(ParcMotionLabel *h, int32_t hands, int32_t correct_pen, int32_t use_ground, float ground_height,
                               int32_t keep_existing) {
    PARC_TRY(tool::check_loaded("mlabel", h, &ParcMotionLabel::batch));
    if (use_ground && !std::isfinite(ground_height)) return fail(PARC_ERR_INVALID, "mlabel: ground_height must be finite");
    ParcMotionLabel::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    mlabel::Cfg G{};
    G.eps = h->eps; G.ground = use_ground != 0; G.ground_height = use_ground ? ground_height : 0.f;
    G.hands = hands && !use_ground; G.correct_pen = correct_pen != 0; G.keep_existing = keep_existing != 0;
    HIPCHK(hipEventRecord(h->ev[0], 0));
    PARC_TRY(tool::launch(mlabel::k_mlabel_feet, dim3(blocks(b.F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W, G));
    HIPCHK(hipEventRecord(h->ev[1], 0));
    if (G.hands)
        PARC_TRY(tool::launch(mlabel::k_mlabel_hands, dim3(blocks(b.F, mlabel::HAND_WAVES)), dim3(64 * mlabel::HAND_WAVES), 0, 0, h->d_model, b.K,
                              b.W, G));
    HIPCHK(hipEventRecord(h->ev[2], 0));
    HIPCHK(hipEventSynchronize(h->ev[2]));
    PARC_TRY(h->ev.elapsed(h->kernel_ms[0], 0, 1));
    PARC_TRY(h->ev.elapsed(h->kernel_ms[1], 1, 2));
    if (!G.hands) h->kernel_ms[1] = 0.f;
    b.ran = true;
    return PARC_OK;
}

namespace mlabel {
static int to_host(const ParcMotionLabel *h, float *dst, const float *src, long long n) {
    if (!dst) return PARC_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}
}  // namespace mlabel

extern "C" int parc_mlabel_get_frames(ParcMotionLabel *h, float *root_pos, float *contacts) {
    PARC_TRY(tool::check_ran("mlabel", h, &ParcMotionLabel::batch));
    if (!root_pos || !contacts) return fail(PARC_ERR_INVALID, "mlabel: null output");
    const ParcMotionLabel::Batch &b = *h->batch;
    PARC_TRY(mlabel::to_host(h, root_pos, b.W.out_root_pos, 3 * b.F));
    return mlabel::to_host(h, contacts, b.W.out_contacts, b.F * h->host_model.B);
}

extern "C" int parc_mlabel_get_gap(ParcMotionLabel *h, float *gap) {
    PARC_TRY(tool::check_ran("mlabel", h, &ParcMotionLabel::batch));
    return mlabel::to_host(h, gap, h->batch->W.gap, 2 * h->batch->F);
}

extern "C" int parc_mlabel_get_lift(ParcMotionLabel *h, float *lift) {
    PARC_TRY(tool::check_ran("mlabel", h, &ParcMotionLabel::batch));
    return mlabel::to_host(h, lift, h->batch->W.lift, h->batch->F);
}

extern "C" int parc_mlabel_get_hand_sd(ParcMotionLabel *h, float *hand_sd) {
    PARC_TRY(tool::check_ran("mlabel", h, &ParcMotionLabel::batch));
    return mlabel::to_host(h, hand_sd, h->batch->W.hand_sd, 2 * h->batch->F);
}

extern "C" int parc_mlabel_resample(ParcMotionLabel *h, const int64_t *out_off, const float *times, const float *lengths, float *root_pos,
                                    float *root_rot, float *joint_rot, float *contacts) {
    PARC_TRY(tool::check_loaded("mlabel", h, &ParcMotionLabel::batch));
    if (!out_off || !times || !lengths || !root_pos || !root_rot || !joint_rot || !contacts) return fail(PARC_ERR_INVALID, "mlabel: null argument");
    const ParcMotionLabel::Batch &b = *h->batch;
    const int C = b.K.C, B = h->host_model.B;
    if (out_off[0] != 0) return fail(PARC_ERR_INVALID, "mlabel: offsets must start at 0");
    std::vector<int> out_clip;
    for (int i = 0; i < C; ++i) {
        const long long n = out_off[i + 1] - out_off[i];
        if (n < 1) return fail(PARC_ERR_INVALID, "mlabel: clip " + std::to_string(i) + " has no output frames");
        if (!(lengths[i] > 0.f) || !std::isfinite(lengths[i])) return fail(PARC_ERR_INVALID, "mlabel: clip " + std::to_string(i) + ": length must be > 0");
        out_clip.insert(out_clip.end(), (size_t)n, i);
    }
    const long long N = out_off[C];
    if (N > 0x7fffffffLL) return fail(PARC_ERR_INVALID, "mlabel: at most 2^31 - 1 output frames");
    HIPCHK(hipSetDevice(h->device));
    DeviceArena mem;                                          // of this call
    mlabel::Resample R{};
    R.N = N;
    PARC_TRY(mem.alloc(R.out_clip, N, out_clip.data()));
    PARC_TRY(mem.alloc(R.times, N, times));
    PARC_TRY(mem.alloc(R.length, (long long)C, lengths));
    PARC_TRY(mem.alloc(R.root_pos, 3 * N));
    PARC_TRY(mem.alloc(R.root_rot, 4 * N));
    PARC_TRY(mem.alloc(R.jrot, 4 * N * (B - 1) + 1));
    PARC_TRY(mem.alloc(R.contacts, N * B));
    HIPCHK(hipEventRecord(h->ev[3], 0));
    PARC_TRY(tool::launch(mlabel::k_mlabel_resample, dim3(blocks(N, 64)), dim3(64), 0, 0, b.K, R, B));
    HIPCHK(hipEventRecord(h->ev[4], 0));
    HIPCHK(hipMemcpy(root_pos, R.root_pos, (size_t)N * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(root_rot, R.root_rot, (size_t)N * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (B > 1) HIPCHK(hipMemcpy(joint_rot, R.jrot, (size_t)N * 4 * (B - 1) * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(contacts, R.contacts, (size_t)N * B * sizeof(float), hipMemcpyDeviceToHost));
    return h->ev.elapsed(h->kernel_ms[2], 3, 4);
}

extern "C" int parc_mlabel_kernel_times(ParcMotionLabel *h, float *ms3) {
    return tool::stored_times("mlabel", h, &ParcMotionLabel::kernel_ms, ms3);
}
