// Prefetch phase of k_env_post: what a lane derives from its index and from constants of the handle (B, S, D, R, the tile radius) only,
// formed once on the host instead of by every env-wave of every step.  Shared by the kernel and a host build
// (tests/test_env_post_lanetab_cpu.py), hence free of anything but integer arithmetic.
//
// One 16-byte entry per lane (one load whose address needs nothing but the lane index).  Every index in it is in bounds for EVERY
// lane: a lane without an item of its own gets slot 0 / sample 0 / cell (0, 0), so that the kernel loads without a branch and without
// a default value; what such a lane loads is never consumed (the consumers test the item, the lane's role or the store mask as before).
//   w0  [0,8) item of pass A, [8,16) item of pass B: row * 16 + slot as int8, -1 = none (parc_rowmap.hpp)
//       [16,18)                record slot of the contact load from frame i1, less 16 (contacts are slots 16..19)
//       [18,24)                float offset of the lane's contact force (3 (lane - 32); 0 = no force of its own)
//       [24,30)                the lane's dof, clamped to D - 1
//   w1  [0,5) [5,10) [10,15)   4 x the sample whose frame blend the lane reads (the byte address of the lane shuffle): pass A, pass B,
//                              contact / velocity block
//       [15,19) [19,23)        record slot of the lane's row load: pass A, pass B (0..15; on row 0 also its slot of the k_env_prep record)
//       [23,28)                record slot of the contact / velocity load from frame i0 (16..19 contacts, 20.. velocities)
//       [28,30)                role in the aux load: 0 none, 1 root velocity, 2 root angular velocity, 3 contact force of body lane - 32
//   w2  tile cells 0, 1, 2 and w3 [0,20) tile cells 3, 4 (cell i = tile index lane + 64 i): 10 bits each, a | bq << 5 with
//       a = idx / (2 tile_r + 1), bq = idx % (2 tile_r + 1); (0, 0) where the tile has no such cell
//   w3  [20,25) bit i = tile cell i exists; [25,29) how many of the lane's 8 ray slots (ray lane + 64 i) lie inside R.  The kernel reads
//       neither: it stores all five cells (the tile's 320 floats are there whatever its radius) and clamps a ray slot against a scalar
//       (parc_lt_ray_off).  They state which of the lane's loads are its own, for the host test and for a reader of a dumped table.
#pragma once

#include "parc_rowmap.hpp"

#define PARC_LANETAB_WORDS 4
#define PARC_LANETAB_TILE_CELLS 5 // per lane: 5 x 64 = the 320 floats the tile may take
#define PARC_LANETAB_RAY_SLOTS 8  // per lane and pass of the ray loop

#define PARC_LT_ROLE_NONE 0
#define PARC_LT_ROLE_ROOT_VEL 1
#define PARC_LT_ROLE_ROOT_ANG_VEL 2
#define PARC_LT_ROLE_FORCE 3

struct alignas(16) ParcLaneEntry { unsigned w[PARC_LANETAB_WORDS]; };

PARC_ROWMAP_HD unsigned parc_lt_bits(unsigned w, int lo, int n) { return (w >> lo) & ((1u << n) - 1u); }
// accessors: the one place that knows the packing (kernel, fill and test go through them)
PARC_ROWMAP_HD int parc_lt_item(const unsigned *w, int pass) { return (int)(w[0] << (pass == 0 ? 24 : 16)) >> 24; }
PARC_ROWMAP_HD unsigned parc_lt_src4(const unsigned *w, int which) { return parc_lt_bits(w[1], 5 * which, 5); } // which: 0 pass A, 1 pass B, 2 contact / velocity
PARC_ROWMAP_HD unsigned parc_lt_row_slot(const unsigned *w, int pass) { return parc_lt_bits(w[1], 15 + 4 * pass, 4); }
PARC_ROWMAP_HD unsigned parc_lt_cv_slot0(const unsigned *w) { return parc_lt_bits(w[1], 23, 5); }
PARC_ROWMAP_HD unsigned parc_lt_cv_slot1(const unsigned *w) { return 16u + parc_lt_bits(w[0], 16, 2); }
PARC_ROWMAP_HD unsigned parc_lt_role(const unsigned *w) { return parc_lt_bits(w[1], 28, 2); }
PARC_ROWMAP_HD unsigned parc_lt_force_off(const unsigned *w) { return parc_lt_bits(w[0], 18, 6); }
PARC_ROWMAP_HD unsigned parc_lt_dof(const unsigned *w) { return parc_lt_bits(w[0], 24, 6); }
PARC_ROWMAP_HD unsigned parc_lt_cell(const unsigned *w, int i) { return i < 3 ? parc_lt_bits(w[2], 10 * i, 10) : parc_lt_bits(w[3], 10 * (i - 3), 10); }
PARC_ROWMAP_HD unsigned parc_lt_cell_a(const unsigned *w, int i) { return parc_lt_cell(w, i) & 31u; }
PARC_ROWMAP_HD unsigned parc_lt_cell_b(const unsigned *w, int i) { return parc_lt_cell(w, i) >> 5; }
PARC_ROWMAP_HD unsigned parc_lt_cell_valid(const unsigned *w, int i) { return parc_lt_bits(w[3], 20 + i, 1); }
PARC_ROWMAP_HD unsigned parc_lt_nray(const unsigned *w) { return parc_lt_bits(w[3], 25, 4); }

// Ray slot i of a lane (ray lane + 64 i of a pass of the ray loop) as a byte offset into the float2 ray points, clamped to the last ray:
// 8 (min(lane, R - 1 - 64 i) + 64 i), the bound a scalar.  top < 0: the slot lies past R on every lane and is not loaded.
PARC_ROWMAP_HD int parc_lt_ray_top(int R, int i) { return 8 * (R - 1 - 64 * i); }
PARC_ROWMAP_HD unsigned parc_lt_ray_off(int lane, int i, int top) {
    const unsigned l8 = 8u * (unsigned)lane;
    return 512u * (unsigned)i + (l8 < (unsigned)top ? l8 : (unsigned)top);
}

// Fills tab[64].  tile_r < 0 (no tile: before a terrain is loaded, or a ray fan too wide for it) leaves every tile cell at (0, 0), invalid.
// false = a value does not fit its field (the caller's limits are wrong).
inline bool parc_lanetab_fill(ParcLaneEntry *tab, int B, int S, int D, int R, int tile_r, unsigned row_mul, unsigned tile_mul) {
    if (B < 2 || B > 15 || S < 0 || S > 6 || D < 1 || D > 40 || R < 1 || tile_r > 15) return false;
    const int TW = 2 * tile_r + 1, ncell = tile_r >= 0 ? TW * TW : 0;
    if (ncell > 64 * PARC_LANETAB_TILE_CELLS) return false;
    const int nvel = 2 + (D + 3) / 4;
    if (20 + nvel > 32) return false; // the velocity block ends with the record
    for (int lane = 0; lane < 64; ++lane) {
        unsigned *w = tab[lane].w;
        for (int i = 0; i < PARC_LANETAB_WORDS; ++i) w[i] = 0u;
        const int item[2] = {parc_rowmap_item<true>(lane, B, 2 + S, row_mul), parc_rowmap_item<false>(lane, B, 2 + S, row_mul)};
        w[0] = ((unsigned)item[0] & 0xffu) | (((unsigned)item[1] & 0xffu) << 8);
        for (int p = 0; p < 2; ++p) {
            const int it = item[p] > 0 ? item[p] : 0, r = it >> 4;
            w[1] |= (unsigned)(4 * (r > 1 ? r - 1 : 0)) << (5 * p); // row 1 = sample 0 (the reference at t), row r = look-ahead target r - 1
            w[1] |= (unsigned)(it & 15) << (15 + 4 * p);
        }
        const bool contact = lane < 4 * (1 + S), vel = !contact && lane >= 32 && lane < 32 + nvel;
        w[1] |= (unsigned)(4 * (contact ? lane >> 2 : 0)) << 10;
        w[1] |= (unsigned)(contact ? 16 + (lane & 3) : vel ? 20 + (lane - 32) : 16) << 23;
        w[0] |= (unsigned)(contact ? lane & 3 : 0) << 16;
        const bool force = lane >= 32 && lane < 32 + B;
        w[1] |= (unsigned)(lane == 30 ? PARC_LT_ROLE_ROOT_VEL : lane == 31 ? PARC_LT_ROLE_ROOT_ANG_VEL : force ? PARC_LT_ROLE_FORCE : PARC_LT_ROLE_NONE) << 28;
        w[0] |= (unsigned)(force ? 3 * (lane - 32) : 0) << 18;
        w[0] |= (unsigned)(lane < D ? lane : D - 1) << 24;
        for (int i = 0; i < PARC_LANETAB_TILE_CELLS; ++i) {
            const int idx = lane + 64 * i;
            if (idx >= ncell) continue;
            const unsigned a = ((unsigned)idx * tile_mul) >> 16, bq = (unsigned)idx - a * (unsigned)TW;
            if (a > 31u || bq > 31u) return false;
            w[i < 3 ? 2 : 3] |= (a | bq << 5) << (10 * (i < 3 ? i : i - 3));
            w[3] |= 1u << (20 + i);
        }
        unsigned nray = 0;
        for (int i = 0; i < PARC_LANETAB_RAY_SLOTS; ++i) nray += lane + 64 * i < R ? 1u : 0u;
        w[3] |= nray << 25;
    }
    return true;
}
