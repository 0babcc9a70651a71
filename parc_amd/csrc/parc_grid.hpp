// parc_grid.hpp — the heightfield helpers that more than one motion tool uses (the optimiser, the analyser, the sampler and the
// augmenter): the reference's float -> int64 conversion, its grid index and its box SDF.  What one tool alone
// uses (sd_box_grad and patch_sdf of the optimiser, terrain_sdf and the linspace Axis of the analyser, which the rollout selection takes from the analyser's header) stays with that tool.
#pragma once
#include <hip/hip_runtime.h>

#include "parc_math.hpp"

namespace parc {

// torch's .to(int64) of a floor / ceil on x86: NaN and out-of-range give INT64_MIN (then clamped like every other index)
__device__ __forceinline__ long long to_i64(float v) {
    return (v >= -9.0e18f && v <= 9.0e18f) ? (long long)v : (long long)(-9223372036854775807LL - 1);
}

// get_grid_index (terrain_util.py:146-152): torch.round (half to even) of a true fp32 division, .to(int64), clamp to [0, dims - 1]
__device__ __forceinline__ long long grid_index(float p, float mn, float d, long long dim) {
    long long i = to_i64(rintf((p - mn) / d));
    i = i < dim - 1 ? i : dim - 1;
    return i > 0 ? i : 0;
}

// sdBox (geom_util.py:124-145) of a point relative to the box centre
__device__ __forceinline__ float sd_box(V3 p, V3 h) {
    const float qx = fabsf(p.x) - h.x, qy = fabsf(p.y) - h.y, qz = fabsf(p.z) - h.z;
    const float px = fmaxf(qx, 0.f), py = fmaxf(qy, 0.f), pz = fmaxf(qz, 0.f);
    return sqrtf(px * px + py * py + pz * pz) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.f);
}

}  // namespace parc
