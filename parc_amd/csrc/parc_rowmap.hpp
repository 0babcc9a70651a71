// Row phase of k_env_post: which (row, slot) item a lane works on in each of the two passes.  Shared by the kernel and a host build
// (tests/test_env_post_rowmap_cpu.py), hence free of anything but integer arithmetic.
//
// An env has rows r in [0, rows) (rows = 2 + S <= 8: character, reference, S look-ahead targets) of 16 slots: slot 0 = root rotation,
// slots 1..B-1 = joint rotations, slot 15 = root position.  The two root items of a row need code of their own (position lerp + loop
// offset, heading products); with one row per 16 lanes that code ran in both passes for two lanes of a row each.  Here all root items
// share pass A, and pass B holds joint items only:
//   pass A: lanes 0..7 = (row lane, slot 0), lanes 8..15 = (row lane - 8, slot 15), lanes 16..63 = joint items 0..47
//   pass B: lanes 0..63 = joint items 48..111
// joint item j = (row j / (B-1), slot 1 + j % (B-1)); the quotient is a multiply-shift with a constant fixed when the env is created.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PARC_ROWMAP_HD __host__ __device__ __forceinline__
#else
#define PARC_ROWMAP_HD inline
#endif

#define PARC_ROWMAP_ROOT_LANES 16                             // pass A: 8 root rotations + 8 root positions
#define PARC_ROWMAP_JOINTS_A (64 - PARC_ROWMAP_ROOT_LANES)    // joint items of pass A
#define PARC_ROWMAP_MAX_JOINT_ITEMS (PARC_ROWMAP_JOINTS_A + 64) // = 8 rows x 14 joints

// j / (B-1) == (j * mul) >> 16 for every j < PARC_ROWMAP_MAX_JOINT_ITEMS (parc_rowmap_mul_ok; 0 when there is no joint)
PARC_ROWMAP_HD unsigned parc_rowmap_mul(int B) { return B > 1 ? (65536u + (unsigned)(B - 1) - 1u) / (unsigned)(B - 1) : 0u; }

PARC_ROWMAP_HD bool parc_rowmap_mul_ok(int B, unsigned mul) {
    if (B <= 1) return true;
    for (unsigned j = 0; j < PARC_ROWMAP_MAX_JOINT_ITEMS; ++j)
        if (((j * mul) >> 16) != j / (unsigned)(B - 1)) return false;
    return true;
}

// The item of `lane` in pass A (ROOT_ITEMS) or pass B, as row * 16 + slot (its index into the 8 x 16 quaternion rows); -1 = the lane has none.
template <bool ROOT_ITEMS>
PARC_ROWMAP_HD int parc_rowmap_item(int lane, int B, int rows, unsigned mul) {
    if (ROOT_ITEMS && lane < PARC_ROWMAP_ROOT_LANES) return (lane & 7) < rows ? 16 * (lane & 7) + (lane < 8 ? 0 : 15) : -1;
    const int j = ROOT_ITEMS ? lane - PARC_ROWMAP_ROOT_LANES : lane + PARC_ROWMAP_JOINTS_A;
    const int row = (int)(((unsigned)j * mul) >> 16);
    return j < rows * (B - 1) ? 16 * row + 1 + (j - row * (B - 1)) : -1;
}
