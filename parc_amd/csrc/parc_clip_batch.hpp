// parc_clip_batch.hpp — the clip batch of the motion tools (parc_mopt_*, parc_mterr_*, parc_msamp_*, parc_maug_*):
// the device views of a packed ParcMotionOptClips batch that the kernels take by value, and the host code that validates and uploads
// one.  No kernel lives here.
//
// ClipArrays is what every tool reads; FrameClips adds the two per-frame / per-clip arrays of the optimiser and the analyser.  A tool
// with arrays of its own derives from these (the optimiser's Clips).  `pre` is the caller's message prefix ("mopt", "mterr", "msamp", "maug");
// the functions know nothing else about their caller.  What only one module checks or uploads stays in that module.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"

struct ClipArrays {                     // device pointers of one batch
    int C;
    long long F;
    const long long *frame_off, *hf_off;
    const float *hf_geom, *hf;
    const float *src_root_pos, *src_root_rot, *src_jrot, *contacts;   // [F][3], [F][4], [F][B-1][4], [F][B]
    const int *hf_dims;                 // last, beside FrameClips::frame_clip: the kernels that read dims[frame_clip[f]] then fetch
};                                      // both pointers with one scalar load (k_mterr_gather: DESIGN.md section 1 has the measurement)

struct FrameClips : ClipArrays {
    const int *frame_clip;              // [F] the clip of every frame
    const float *hf_min;                // [C] torch.min(hf).item()
};

// ---- validation and upload -------------------------------------------------------------------------------------------------------
struct ClipBatch {                        // what clip_batch_clips derives from a valid batch
    int C = 0;
    long long F = 0, ncell = 0;           // frames and heightfield cells of all clips
    std::vector<int> frame_clip;          // [F] the clip of every frame
    std::vector<float> hf_min;            // [C] torch.min(hf).item()
};

// the batch as a whole: at least one clip, the nine shared arrays present, frame and cell offsets starting at 0
static int clip_batch_arrays(const char *pre, const ParcMotionOptClips *c) {
    if (c->num_clips < 1) return fail(PARC_ERR_INVALID, std::string(pre) + ": num_clips must be >= 1");
    if (!c->frame_off_host || !c->hf_off_host || !c->hf_dims_host || !c->hf_geom_host || !c->hf_host || !c->root_pos_host ||
        !c->root_rot_host || !c->joint_rot_host || !c->contacts_host)
        return fail(PARC_ERR_INVALID, std::string(pre) + ": null clip array");
    if (c->frame_off_host[0] != 0 || c->hf_off_host[0] != 0) return fail(PARC_ERR_INVALID, std::string(pre) + ": offsets must start at 0");
    return PARC_OK;
}

// every clip of a batch that passed clip_batch_arrays: frames, heightfield dims against the offsets, cell size; fills `b`
static int clip_batch_clips(const char *pre, const ParcMotionOptClips *c, ClipBatch &b) {
    const int C = c->num_clips;
    b = ClipBatch{};
    b.hf_min.resize((size_t)C);
    for (int i = 0; i < C; ++i) {
        const long long nf = c->frame_off_host[i + 1] - c->frame_off_host[i];
        const long long X = c->hf_dims_host[2 * i], Y = c->hf_dims_host[2 * i + 1];
        if (nf < 1) return fail(PARC_ERR_INVALID, std::string(pre) + ": clip " + std::to_string(i) + " has no frames");
        if (X < 1 || Y < 1 || c->hf_off_host[i + 1] - c->hf_off_host[i] != X * Y)
            return fail(PARC_ERR_INVALID, std::string(pre) + ": heightfield dims / offsets disagree");
        if (!(c->hf_geom_host[4 * i + 2] > 0.f) || !(c->hf_geom_host[4 * i + 3] > 0.f)) return fail(PARC_ERR_INVALID, std::string(pre) + ": dx must be > 0");
        float mn = INFINITY;                                  // torch.min(hf).item()
        for (long long k = c->hf_off_host[i]; k < c->hf_off_host[i + 1]; ++k) mn = fminf(mn, c->hf_host[k]);
        b.hf_min[(size_t)i] = mn;
        b.frame_clip.insert(b.frame_clip.end(), (size_t)nf, i);
    }
    b.C = C; b.F = c->frame_off_host[C]; b.ncell = c->hf_off_host[C];
    if (b.F > 0x7fffffffLL) return fail(PARC_ERR_INVALID, std::string(pre) + ": at most 2^31 - 1 frames per batch");
    return PARC_OK;
}

// K.C, K.F and the nine arrays of K, allocated from `mem`; B = bodies of the character
static int clip_batch_upload(DeviceArena &mem, ClipArrays &K, const ParcMotionOptClips *c, const ClipBatch &b, int B) {
    const long long C = b.C, F = b.F;
    K.C = b.C; K.F = F;
    PARC_TRY(mem.alloc(K.frame_off, C + 1, c->frame_off_host));
    PARC_TRY(mem.alloc(K.hf_off, C + 1, c->hf_off_host));
    PARC_TRY(mem.alloc(K.hf_dims, 2 * C, c->hf_dims_host));
    PARC_TRY(mem.alloc(K.hf_geom, 4 * C, c->hf_geom_host));
    PARC_TRY(mem.alloc(K.hf, b.ncell, c->hf_host));
    PARC_TRY(mem.alloc(K.src_root_pos, 3 * F, c->root_pos_host));
    PARC_TRY(mem.alloc(K.src_root_rot, 4 * F, c->root_rot_host));
    PARC_TRY(mem.alloc(K.src_jrot, 4 * F * (B - 1), c->joint_rot_host));
    PARC_TRY(mem.alloc(K.contacts, F * B, c->contacts_host));
    return PARC_OK;
}

// K.frame_clip and K.hf_min from what clip_batch_clips derived
static int clip_batch_upload_frames(DeviceArena &mem, FrameClips &K, const ClipBatch &b) {
    PARC_TRY(mem.alloc(K.frame_clip, b.F, b.frame_clip.data()));
    return mem.alloc(K.hf_min, b.C, b.hf_min.data());
}
