// parc_motion_edit.hpp — hesitation-frame removal on gfx950 (parc_medit_*, include/parc_env.h).
//
// The reference's medit_lib.remove_hesitation_frames (motion_edit_lib.py:804-878) for a whole batch of clips: frame j is a hesitation
// frame when an earlier frame i that is not one itself has all its body positions within hesitation_val of frame j's (one norm over
// the B x 3 numbers); runs of at least hesitation_min_seq_len consecutive hesitation frames are dropped, the other frames are kept as
// they are.  All clips of a batch go through:
//   k_medit_fk      lane per frame: FK (parc_char.hpp's fk_frame) into a per-frame workspace, then the body positions again
//                   frame-minor ([clip][B * 3][T]), so that lanes over frames read them contiguously
//   k_medit_pairs   wave per anchor frame i, lanes over j: d(i, j) < hesitation_val for j > i, 64 pairs per __ballot = one 64-bit word
//                   of row i of the clip's upper-triangular pair mask (the words left of the diagonal are written as 0)
//   k_medit_scan    wave per clip: the reference's ordered scan over the rows (lane l holds word l of the flag set; row i is ORed in
//                   when bit i is clear; the row loads do not depend on the flags and run a chunk ahead), the run filter, and the
//                   kept source indices by a ballot prefix count
//   k_medit_gather  lane per output number: the kept rows of the four frame arrays, copied
// No float reduction whose order depends on the batch: a clip's results are bit-identical alone or in any batch.
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
#include "parc_clip_batch.hpp"
#include "parc_tool_handle.hpp"

namespace medit {
using namespace parc;

typedef unsigned long long u64;
constexpr int MAX_T = PARC_MEDIT_MAX_FRAMES;
constexpr int WORDS = PARC_MEDIT_FLAG_WORDS;   // flag words per clip: one per lane of the scan's wave
constexpr int PAIR_WAVES = 4;                  // anchor rows per block of k_medit_pairs
constexpr int SCAN_AHEAD = 8;                  // rows of the pair mask that k_medit_scan loads before it uses the first
static_assert(WORDS == 64 && MAX_T == 64 * WORDS, "the scan keeps one flag word per lane of a wave64");

struct Cfg {                           // by value
    float val;                         // hesitation_val
    int min_len;                       // hesitation_min_seq_len
};

struct Work {
    float *pos, *rot;                  // [F][B][3], [F][B][4]: fk_frame's outputs
    float *pos_t;                      // per clip at frame_off[c] * B * 3: [B * 3][T], frame-minor
    const long long *row_off;          // [C + 1] offsets, in words, of the clips' pair masks
    u64 *rows;                         // per clip at row_off[c]: [T][ceil(T / 64)], bit j & 63 of word j >> 6 of row i: j > i and d(i, j) < val
    u64 *flags_raw, *flags;            // [C][WORDS] the flag set after the scan, and after the run filter
    int *kept;                         // [F]: clip c's kept source frames at frame_off[c], ascending, first count[c] used
    int *count;                        // [C]
    const int *src;                    // [total kept] the batch frame of every output frame (host, after a run)
    float *out_root_pos, *out_root_rot, *out_jrot, *out_contacts;   // [total kept] rows
};

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ void k_medit_fk(const CharTree *Mp, FrameClips K, Work W) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const CharTree &M = *Mp;
    const int B = M.B;
    float *pos = W.pos + f * B * 3;
    // fk_frame reads joint j's rotation at base + 4 j for j >= 1 only
    fk_frame(M, ld3(K.src_root_pos + 3 * f), ld4(K.src_root_rot + 4 * f), K.src_jrot + f * (B - 1) * 4 - 4, pos, W.rot + f * B * 4);
    const int c = K.frame_clip[f];
    const long long f0 = K.frame_off[c], T = K.frame_off[c + 1] - f0;
    float *pt = W.pos_t + f0 * B * 3 + (f - f0);
    for (int k = 0; k < B * 3; ++k) pt[k * T] = pos[k];
}

__global__ void __launch_bounds__(64 * PAIR_WAVES) k_medit_pairs(FrameClips K, Work W, Cfg G, int B3) {
    // the wave's anchor frame: the same in every lane, so its clip, offsets and positions are scalar loads
    const long long f = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long long)blockIdx.x * PAIR_WAVES;
    if (f >= K.F) return;
    const int lane = threadIdx.x & 63;
    const int c = K.frame_clip[f];
    const long long f0 = K.frame_off[c];
    const int T = (int)(K.frame_off[c + 1] - f0), i = (int)(f - f0), nw = (T + 63) >> 6;
    const float *pt = W.pos_t + f0 * B3;
    u64 *row = W.rows + W.row_off[c] + (long long)i * nw;
    for (int w = 0; w < nw; ++w) {
        const int j = w * 64 + lane;
        bool hit = false;
        if (w >= (i >> 6)) {                                  // wave-uniform: the words left of the diagonal hold no pair
            const int jc = j < T ? j : T - 1;                 // the last word's spare lanes read the last frame; their bits are masked
            float s = 0.f;
            for (int k = 0; k < B3; ++k) {
                const float d = pt[(long long)k * T + jc] - pt[(long long)k * T + i];
                s += d * d;
            }
            hit = j > i && j < T && sqrtf(s) < G.val;        // torch.linalg.norm(body_pos[j] - body_pos[i]) < hesitation_val
        }
        const u64 m = __ballot(hit);
        if (lane == 0) row[w] = m;
    }
}

__global__ void __launch_bounds__(64) k_medit_scan(FrameClips K, Work W, Cfg G) {
    __shared__ u64 s_flag[WORDS];
    const int c = blockIdx.x, lane = threadIdx.x;
    const long long f0 = K.frame_off[c];
    const int T = (int)(K.frame_off[c + 1] - f0), nw = (T + 63) >> 6;
    const u64 *rows = W.rows + W.row_off[c];
    // the ordered scan.  flag = word `lane` of the flag set; cur = the word that holds bit i, the same in every lane: with the
    // diagonal word of row i (a uniform load) it carries the only dependence from step to step, and the vector OR hangs off it
    u64 flag = 0, cur = 0;
    for (int i0 = 0; i0 < T; i0 += SCAN_AHEAD) {
        u64 v[SCAN_AHEAD], d[SCAN_AHEAD];
#pragma unroll
        for (int q = 0; q < SCAN_AHEAD; ++q) {
            const int i = i0 + q;
            v[q] = (i < T && lane < nw) ? rows[(long long)i * nw + lane] : 0ull;
            d[q] = i < T ? rows[(long long)i * nw + (i >> 6)] : 0ull;
        }
#pragma unroll
        for (int q = 0; q < SCAN_AHEAD; ++q) {
            const int i = i0 + q;
            if (i < T) {
                if ((i & 63) == 0) {                          // a new word: every earlier row's bits for it are in its owner lane
                    const unsigned lo = __shfl((unsigned)flag, i >> 6), hi = __shfl((unsigned)(flag >> 32), i >> 6);
                    cur = ((u64)hi << 32) | lo;
                }
                if (!((cur >> (i & 63)) & 1ull)) { flag |= v[q]; cur |= d[q]; }
            }
        }
    }
    W.flags_raw[(long long)c * WORDS + lane] = flag;
    s_flag[lane] = flag;
    __syncthreads();
    // the run filter: runs of consecutive flagged frames shorter than min_len are unflagged again.  One lane walks the frames (the scan
    // above is as long); a run's length is known at its end, where its bits are cleared if it is too short
    if (lane == 0) {
        int start = -1;
        for (int j = 0; j <= T; ++j) {
            const bool on = j < T && ((s_flag[j >> 6] >> (j & 63)) & 1ull);
            if (on && start < 0) start = j;
            if (!on && start >= 0) {
                if (j - start < G.min_len)
                    for (int k = start; k < j; ++k) s_flag[k >> 6] &= ~(1ull << (k & 63));
                start = -1;
            }
        }
    }
    __syncthreads();
    const u64 fl = s_flag[lane];
    W.flags[(long long)c * WORDS + lane] = fl;
    // the kept frames, ascending: per word a ballot and a prefix count
    int base = 0;
    for (int w = 0; w < nw; ++w) {
        const int j = w * 64 + lane;
        const bool keep = j < T && !((s_flag[w] >> lane) & 1ull);
        const u64 m = __ballot(keep);
        if (keep) W.kept[f0 + base + __popcll(m & ((1ull << lane) - 1ull))] = j;
        base += __popcll(m);
    }
    for (int j = base + lane; j < T; j += 64) W.kept[f0 + j] = -1;
    if (lane == 0) W.count[c] = base;
}

// out row o = source row src[o], for the four frame arrays at once: e indexes the 3 + 4 + 4 (B - 1) + B numbers of a frame
__global__ void k_medit_gather(ClipArrays K, Work W, long long n_out, int B) {
    const int J4 = 4 * (B - 1), len = 7 + J4 + B;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_out * len) return;
    const long long o = idx / len, f = W.src[o];
    const int e = (int)(idx - o * len);
    if (e < 3) W.out_root_pos[3 * o + e] = K.src_root_pos[3 * f + e];
    else if (e < 7) W.out_root_rot[4 * o + e - 3] = K.src_root_rot[4 * f + e - 3];
    else if (e < 7 + J4) W.out_jrot[J4 * o + e - 7] = K.src_jrot[J4 * f + e - 7];
    else W.out_contacts[B * o + e - 7 - J4] = K.contacts[B * f + e - 7 - J4];
}

}  // namespace medit

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcMotionEdit : tool::CharHandle<parc::CharTree, DeviceEvents<6>> {   // mem: d_model
    struct Batch {                        // what one parc_medit_set_clips loads; a batch is loaded when the handle holds one
        DeviceArena mem;
        FrameClips K{};
        medit::Work W{};
        int *d_src = nullptr;             // W.src, writable
        std::vector<long long> frame_off, row_off;
        std::vector<int> counts, kept, src;
        long long F = 0, total = 0;
        bool ran = false;
    };
    medit::Cfg cfg{};
    std::unique_ptr<Batch> batch;
    float kernel_ms[4] = {};
};

extern "C" void parc_medit_destroy(ParcMotionEdit *h) { tool::destroy(h); }

extern "C" int parc_medit_create(const ParcMotionEditParams *p, ParcMotionEdit **out) {
    PARC_TRY(tool::create_args("medit", "ParcMotionEditParams", p, out, 1, true));
    if (!std::isfinite(p->hesitation_val)) return fail(PARC_ERR_INVALID, "medit: hesitation_val must be finite");
    if (p->hesitation_min_seq_len < 1) return fail(PARC_ERR_INVALID, "medit: hesitation_min_seq_len must be >= 1");
    parc::CharTree M;
    PARC_TRY(tool::char_tree("medit", p->model, M));
    return tool::create("medit", p->device, M, out, [&](ParcMotionEdit &h) -> int {
        h.cfg.val = p->hesitation_val; h.cfg.min_len = p->hesitation_min_seq_len;
        return PARC_OK;
    });
}

// as parc_mopt_set_clips: validate; release the old batch; build the new one in a local; install it last
extern "C" int parc_medit_set_clips(ParcMotionEdit *h, const ParcMotionOptClips *c) {
    if (!h || !c) return fail(PARC_ERR_INVALID, "medit: null argument");
    PARC_TRY(clip_batch_arrays("medit", c));
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("medit", c, cb));
    const int C = cb.C, B = h->host_model.B;
    const long long F = cb.F;
    std::vector<long long> row_off((size_t)C + 1, 0);
    for (int i = 0; i < C; ++i) {
        const long long T = c->frame_off_host[i + 1] - c->frame_off_host[i];
        if (T > PARC_MEDIT_MAX_FRAMES)
            return fail(PARC_ERR_INVALID, "medit: clip " + std::to_string(i) + " has " + std::to_string(T) + " frames; at most " +
                                              std::to_string(PARC_MEDIT_MAX_FRAMES) + " are supported");
        row_off[(size_t)i + 1] = row_off[(size_t)i] + T * ((T + 63) / 64);
    }
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<ParcMotionEdit::Batch> nb;
    PARC_TRY(tool::renew("medit", h->batch, nb));
    FrameClips &K = nb->K;
    medit::Work &W = nb->W;
    DeviceArena &mem = nb->mem;
    PARC_TRY(clip_batch_upload(mem, K, c, cb, B));
    PARC_TRY(clip_batch_upload_frames(mem, K, cb));
    PARC_TRY(mem.alloc(W.pos, 3 * F * B));
    PARC_TRY(mem.alloc(W.rot, 4 * F * B));
    PARC_TRY(mem.alloc(W.pos_t, 3 * F * B));
    PARC_TRY(mem.alloc(W.row_off, (long long)C + 1, row_off.data()));
    PARC_TRY(mem.alloc(W.rows, row_off[(size_t)C]));
    PARC_TRY(mem.alloc(W.flags_raw, (long long)C * medit::WORDS));
    PARC_TRY(mem.alloc(W.flags, (long long)C * medit::WORDS));
    PARC_TRY(mem.alloc(W.kept, F));
    PARC_TRY(mem.alloc(W.count, C));
    PARC_TRY(mem.alloc(nb->d_src, F));
    W.src = nb->d_src;
    PARC_TRY(mem.alloc(W.out_root_pos, 3 * F));
    PARC_TRY(mem.alloc(W.out_root_rot, 4 * F));
    PARC_TRY(mem.alloc(W.out_jrot, 4 * F * (B - 1)));
    PARC_TRY(mem.alloc(W.out_contacts, F * B));
    nb->F = F;
    nb->frame_off.assign(c->frame_off_host, c->frame_off_host + C + 1);
    nb->row_off = std::move(row_off);
    nb->counts.assign((size_t)C, 0);
    nb->kept.assign((size_t)F, -1);
    nb->src.assign((size_t)F, 0);
    h->batch = std::move(nb);
    return PARC_OK;
}

extern "C" int parc_medit_run(ParcMotionEdit *h, int32_t *kept_counts, int32_t *kept_inds, int64_t *total_kept) {
    PARC_TRY(tool::check_loaded("medit", h, &ParcMotionEdit::batch));
    ParcMotionEdit::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    const long long F = b.F;
    const int C = b.K.C, B = h->host_model.B;
    HIPCHK(hipEventRecord(h->ev[0], 0));
    PARC_TRY(tool::launch(medit::k_medit_fk, dim3(blocks(F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W));
    HIPCHK(hipEventRecord(h->ev[1], 0));
    PARC_TRY(tool::launch(medit::k_medit_pairs, dim3(blocks(F, medit::PAIR_WAVES)), dim3(64 * medit::PAIR_WAVES), 0, 0, b.K, b.W, h->cfg, 3 * B));
    HIPCHK(hipEventRecord(h->ev[2], 0));
    PARC_TRY(tool::launch(medit::k_medit_scan, dim3((unsigned)C), dim3(64), 0, 0, b.K, b.W, h->cfg));
    HIPCHK(hipEventRecord(h->ev[3], 0));
    HIPCHK(hipMemcpy(b.counts.data(), b.W.count, (size_t)C * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(b.kept.data(), b.W.kept, (size_t)F * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) PARC_TRY(h->ev.elapsed(h->kernel_ms[k], k, k + 1));
    long long tot = 0;                                        // the batch frame of every output frame, clips in order
    for (int c = 0; c < C; ++c) {
        const long long f0 = b.frame_off[(size_t)c], T = b.frame_off[(size_t)c + 1] - f0;
        const int n = b.counts[(size_t)c];
        if (n < 1 || n > T) return fail(PARC_ERR_HIP, "medit: kept count out of range (clip " + std::to_string(c) + ")");
        for (int k = 0; k < n; ++k) {
            const int j = b.kept[(size_t)(f0 + k)];
            if (j < 0 || j >= T) return fail(PARC_ERR_HIP, "medit: kept index out of range (clip " + std::to_string(c) + ")");
            b.src[(size_t)tot++] = (int)(f0 + j);
        }
    }
    HIPCHK(hipMemcpy(b.d_src, b.src.data(), (size_t)tot * sizeof(int), hipMemcpyHostToDevice));
    b.total = tot;
    b.ran = true;
    if (kept_counts) memcpy(kept_counts, b.counts.data(), (size_t)C * sizeof(int));
    if (kept_inds) memcpy(kept_inds, b.kept.data(), (size_t)F * sizeof(int));
    if (total_kept) *total_kept = tot;
    return PARC_OK;
}

extern "C" int parc_medit_get_frames(ParcMotionEdit *h, float *root_pos, float *root_rot, float *joint_rot, float *contacts) {
    PARC_TRY(tool::check_ran("medit", h, &ParcMotionEdit::batch));
    if (!root_pos || !root_rot || !joint_rot || !contacts) return fail(PARC_ERR_INVALID, "medit: null output");
    const ParcMotionEdit::Batch &b = *h->batch;
    const int B = h->host_model.B;
    const long long n = b.total, len = 7 + 4 * (B - 1) + B;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->ev[4], 0));
    PARC_TRY(tool::launch(medit::k_medit_gather, dim3(blocks(n * len, 256)), dim3(256), 0, 0, b.K, b.W, n, B));
    HIPCHK(hipEventRecord(h->ev[5], 0));
    HIPCHK(hipMemcpy(root_pos, b.W.out_root_pos, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(root_rot, b.W.out_root_rot, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (B > 1) HIPCHK(hipMemcpy(joint_rot, b.W.out_jrot, (size_t)n * 4 * (B - 1) * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(contacts, b.W.out_contacts, (size_t)n * B * sizeof(float), hipMemcpyDeviceToHost));
    return h->ev.elapsed(h->kernel_ms[3], 4, 5);
}

extern "C" int parc_medit_get_pair_rows(ParcMotionEdit *h, int32_t clip, uint64_t *rows) {
    PARC_TRY(tool::check_ran("medit", h, &ParcMotionEdit::batch));
    const ParcMotionEdit::Batch &b = *h->batch;
    if (clip < 0 || clip >= b.K.C || !rows) return fail(PARC_ERR_INVALID, "medit: bad pair-row request");
    HIPCHK(hipSetDevice(h->device));
    const long long n = b.row_off[(size_t)clip + 1] - b.row_off[(size_t)clip];
    HIPCHK(hipMemcpy(rows, b.W.rows + b.row_off[(size_t)clip], (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_medit_get_flags(ParcMotionEdit *h, uint64_t *raw, uint64_t *filtered) {
    PARC_TRY(tool::check_ran("medit", h, &ParcMotionEdit::batch));
    const ParcMotionEdit::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)b.K.C * medit::WORDS * sizeof(uint64_t);
    if (raw) HIPCHK(hipMemcpy(raw, b.W.flags_raw, n, hipMemcpyDeviceToHost));
    if (filtered) HIPCHK(hipMemcpy(filtered, b.W.flags, n, hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_medit_kernel_times(ParcMotionEdit *h, float *ms4) {
    return tool::stored_times("medit", h, &ParcMotionEdit::kernel_ms, ms4);
}
