// parc_clip_batch.hpp — host code shared by the handles of the motion tools (parc_mopt_*, parc_mterr_*, parc_msamp_*; DESIGN.md
// section 8d): the fill and upload of mopt::Model from ParcCharModel, and the validation and upload of the part of a packed
// ParcMotionOptClips batch that the optimiser, the analyser and the sampler all read.  No kernel lives here.
//
// `pre` is the caller's message prefix ("mopt", "mterr", "msamp"); the functions know nothing else about their caller.  What only one
// module checks or uploads stays in that module.  mopt::Model and mopt::Clips are defined with the kernels that read them
// (parc_motion_opt.hpp, which includes this file), so the functions that fill them take them as a template parameter.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"

// ---- the character model ---------------------------------------------------------------------------------------------------------
// M = zeros, then B, D and the tree of cm.  The caller has checked num_bodies (and dof_size) against the limits.
template <typename Model> static int model_tree(const char *pre, const ParcCharModel &cm, Model &M) {
    memset(&M, 0, sizeof(M));
    M.B = cm.num_bodies; M.D = cm.dof_size;
    for (int b = 0; b < M.B; ++b) {
        M.parent[b] = cm.parent[b]; M.jtype[b] = cm.joint_type[b]; M.dof_idx[b] = cm.dof_idx[b];
        if (b > 0 && (cm.parent[b] < 0 || cm.parent[b] >= b)) return fail(PARC_ERR_INVALID, std::string(pre) + ": parents must precede their children");
        for (int k = 0; k < 3; ++k) { M.lt[b][k] = cm.local_translation[b][k]; M.axis[b][k] = cm.joint_axis[b][k]; }
        for (int k = 0; k < 4; ++k) M.lr[b][k] = cm.local_rotation[b][k];
    }
    return PARC_OK;
}

// the sample points, grouped by body (pt_start / pt_count), and the contact column of every body; after model_tree
template <typename Model>
static int model_points(const char *pre, Model &M, int num_points, const float *points_host, const int32_t *point_body_host,
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

// the handle's copy of the model on the current device, allocated from `mem`
template <typename Model> static int model_upload(DeviceArena &mem, const Model &M, Model *&d_model) { return mem.alloc(d_model, 1, &M); }

// ---- the clip batch --------------------------------------------------------------------------------------------------------------
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

// K.C, K.F and the nine shared arrays of K, allocated from `mem`; B = bodies of the character
template <typename Clips> static int clip_batch_upload(DeviceArena &mem, Clips &K, const ParcMotionOptClips *c, const ClipBatch &b, int B) {
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
