// The motion table of parc_env_load_motions: the part of MotionLib._load_motion_file (motion_lib.py:255-401) that needs no device.
// Shared by the library and a host build (tests/test_motion_table_cpu.py), hence free of anything but the standard library.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

struct MotionMeta { // 32 B, read by the kernels (frame_blend, parc_common.hpp)
    int start, nframes;
    float length;
    int loop;
    float dx, dy, dz;
    float fps;
};

#define PARC_MOTION_TABLE_MAX_FRAMES ((int64_t)1 << 30)

// The clips of a motion set, checked and tabulated: one MotionMeta and one normalised weight per clip, and the clip of every frame.
// num_frames, fps, loop_modes, weights: [M]; root_pos: [F][3], the clips concatenated.  Returns nullptr, or the message of the first
// clip that is refused; the outputs are written only on success.
inline const char *parc_motion_table(int M, const int32_t *num_frames, const int32_t *fps, const int32_t *loop_modes, const double *weights,
                                     const float *root_pos, std::vector<MotionMeta> &meta_out, std::vector<float> &weights_out,
                                     std::vector<int> &frame_motion_out) {
    int64_t F = 0;
    float wsum = 0.f;
    for (int m = 0; m < M; ++m) {
        if (num_frames[m] < 2) return "every clip needs at least 2 frames";
        if (fps[m] <= 0) return "fps must be positive";
        if (weights[m] < 0) return "motion weights must be >= 0";
        wsum = wsum + (float)weights[m];
        F += num_frames[m];
    }
    if (F > PARC_MOTION_TABLE_MAX_FRAMES) return "too many frames";
    std::vector<MotionMeta> meta((size_t)M);
    std::vector<float> w((size_t)M);
    std::vector<int> frame_motion;
    frame_motion.reserve((size_t)F);
    int start = 0;
    for (int m = 0; m < M; ++m) {
        MotionMeta &mm = meta[(size_t)m];
        const int n = num_frames[m];
        mm.start = start; mm.nframes = n; mm.loop = loop_modes[m]; mm.fps = (float)fps[m];
        mm.length = (float)(1.0 / (double)fps[m] * (double)(n - 1)); // motion_lib.py:305
        const float *rp = root_pos + 3 * (size_t)start;
        mm.dx = rp[3 * (n - 1)] - rp[0]; mm.dy = rp[3 * (n - 1) + 1] - rp[1]; mm.dz = 0.f; // :307-308
        w[(size_t)m] = (float)weights[m] / wsum; // :372
        frame_motion.insert(frame_motion.end(), (size_t)n, m);
        start += n;
    }
    meta_out.swap(meta); weights_out.swap(w); frame_motion_out.swap(frame_motion);
    return nullptr;
}
