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

#include "parc_rowmap.hpp"   // PARC_ROWMAP_HD (with the HIP runtime it needs under hipcc), parc_rowmap_item

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

// ------------------------------------------------------------------------------------------------
// Heading pass of k_env_post: every 3-vector of the observation that is rotated by the inverse heading -- the S root offsets of the
// target rows, the character's root velocity and angular velocity, the K key-body offsets of the character and the S K of the targets --
// goes through ONE quat_rotate stream after the FK phase, one vector per lane.  What a lane rotates and where the result goes depends on
// the lane and on constants of the handle only (S, K, the key bodies, the observation layout), so it is a second 64-entry table, 12 bytes
// per lane (words 0 and 1; word 2 serves the contact / velocity block, below).  Lanes in this order: target roots (lane s = target row
// 2 + s), root velocity, root angular velocity, character keys, target keys.
//
// A wave's quaternion rows, FK positions and root velocities are one LDS block of float4 (PARC_HROT_*_F4 below), so that a source is one
// byte offset into it.  The lane forms (src - sub), rotates it (or not: global_obs) and stores three floats at `dst` of the staged row:
//   w0  [0,12)   byte offset of the source float4 in the block          [16,28) byte offset of the float4 that is subtracted from it
//   w1  [0,14)   byte offset of the destination in the staged observation row
//       [16,24)  4 x the lane whose rotated vector is added to this lane's (the byte address of the lane shuffle): a target key adds the
//                root offset of its row, which lane `row - 2` forms in the same pass
//       [24]     the lane has an item, [25] it adds the shuffled vector (never under global_obs: mgdm_dm_util.py:417)
// The root velocities have no subtrahend: theirs is the block's zero slot (v - (+0) is v bit for bit for every v that is not a NaN).
// A lane without an item holds zeros: offsets that are in bounds, and no store.
// ------------------------------------------------------------------------------------------------
#define PARC_HROT_Q_F4 0      // float4 (*)[16]: 8 rows of quaternions, slot 15 = root position
#define PARC_HROT_FK_F4 128   // 80 float4 of FK positions (the terrain tile before FK)
#define PARC_HROT_RV_F4 208   // root velocity, root angular velocity of the character, a zero vector, one spare
#define PARC_HROT_RV_ZERO 2
#define PARC_HROT_BLOCK_F4 212

struct alignas(4) ParcHrotEntry { unsigned w[3]; };

PARC_ROWMAP_HD unsigned parc_hr_src(const unsigned *w) { return parc_lt_bits(w[0], 0, 12); }
PARC_ROWMAP_HD unsigned parc_hr_sub(const unsigned *w) { return parc_lt_bits(w[0], 16, 12); }
PARC_ROWMAP_HD unsigned parc_hr_dst(const unsigned *w) { return parc_lt_bits(w[1], 0, 14); }
PARC_ROWMAP_HD unsigned parc_hr_add4(const unsigned *w) { return parc_lt_bits(w[1], 16, 8); }
PARC_ROWMAP_HD bool parc_hr_item(const unsigned *w) { return (w[1] >> 24 & 1u) != 0u; }
PARC_ROWMAP_HD bool parc_hr_adds(const unsigned *w) { return (w[1] >> 25 & 1u) != 0u; }

//   w2  the lane's part in the contact / velocity block behind the row passes (the loads are the lane table's, parc_lt_cv_slot0 / 1):
//       [0,16)  kind TAR: byte offset in the observation row of the lane's first contact, 4 (off_tarc + (s - 1) B + 4 c)
//       [16,19) how many of the lane's four contacts (bodies 4 c .. 4 c + 3) are bodies
//       [20,22) kind: 0 none, 1 contacts of sample 0 (the reward's reference contacts: s_refct[4 c ..]), 2 contacts of target s (the
//               observation row; only when that block exists), 3 velocity block (float4 lane - 32 of s_refvel)
//       [24,28) kind REF: c, kind VEL: lane - 32
#define PARC_HR_CV_NONE 0
#define PARC_HR_CV_REF 1
#define PARC_HR_CV_TAR 2
#define PARC_HR_CV_VEL 3
PARC_ROWMAP_HD unsigned parc_hr_cv_off(const unsigned *w) { return parc_lt_bits(w[2], 0, 16); }
PARC_ROWMAP_HD unsigned parc_hr_cv_n(const unsigned *w) { return parc_lt_bits(w[2], 16, 3); }
PARC_ROWMAP_HD unsigned parc_hr_cv_kind(const unsigned *w) { return parc_lt_bits(w[2], 20, 2); }
PARC_ROWMAP_HD unsigned parc_hr_cv_idx(const unsigned *w) { return parc_lt_bits(w[2], 24, 4); }

// w2 of tab[64]: off_tarc = where the target contacts start in the row, tar_contacts = that block exists
inline bool parc_hrot_fill_cv(ParcHrotEntry *tab, int B, int S, int D, int off_tarc, int tar_contacts) {
    if (B < 2 || B > 15 || S < 0 || S > 6 || D < 1 || D > 40) return false;
    const int nvel = 2 + (D + 3) / 4;
    for (int lane = 0; lane < 64; ++lane) {
        unsigned &w = tab[lane].w[2];
        w = 0u;
        const int s = lane >> 2, c = lane & 3, nk = B - 4 * c < 0 ? 0 : B - 4 * c > 4 ? 4 : B - 4 * c;
        if (lane < 4 * (1 + S)) {
            if (nk == 0 || (s > 0 && !tar_contacts)) continue;
            const int off = s > 0 ? 4 * (off_tarc + (s - 1) * B + 4 * c) : 0;
            if (off >= (1 << 16)) return false;
            w = (unsigned)off | (unsigned)nk << 16 | (unsigned)(s == 0 ? PARC_HR_CV_REF : PARC_HR_CV_TAR) << 20 | (unsigned)c << 24;
        } else if (lane >= 32 && lane < 32 + nvel) {
            if (lane - 32 > 11) return false; // s_refvel holds 12 float4
            w = (unsigned)PARC_HR_CV_VEL << 20 | (unsigned)(lane - 32) << 24;
        }
    }
    return true;
}

// Fills tab[64].  key_ids[K] / key_slot[16] as in HierTables (body of key k; body -> its key slot in the targets' FK scratch); oc = offset of
// the character block; tar_obs = the target block exists, tar_contacts = so does the block of the targets' contacts; global_obs = no lane
// adds; nst = length of the staged row = off_tarc (every store of the heading pass must end inside it; the targets' contacts start there).
// false = an item has no lane, or a value does not fit its field or its array.
inline bool parc_hrot_fill(ParcHrotEntry *tab, int B, int S, int D, int K, const int *key_ids, const int *key_slot, int oc, int off_key, int off_tar,
                           int tar_w, int tar_obs, int tar_contacts, int global_obs, int nst) {
    if (B < 2 || B > 15 || S < 0 || S > 6 || K < 0 || K > 8) return false;
    for (int lane = 0; lane < 64; ++lane) tab[lane].w[0] = tab[lane].w[1] = 0u;
    if (!parc_hrot_fill_cv(tab, B, S, D, nst, tar_contacts)) return false;
    int n = 0;
    bool ok = true;
    auto put = [&](int src_f4, int sub_f4, int dst, int add_lane) {
        if (n >= 64 || src_f4 < 0 || src_f4 >= PARC_HROT_BLOCK_F4 || sub_f4 < 0 || sub_f4 >= PARC_HROT_BLOCK_F4 || dst < 0 || dst + 3 > nst || 4 * dst >= (1 << 14)) { ok = false; return; }
        tab[n].w[0] = (unsigned)(16 * src_f4) | (unsigned)(16 * sub_f4) << 16;
        tab[n].w[1] = (unsigned)(4 * dst) | (unsigned)(add_lane >= 0 ? 4 * add_lane : 0) << 16 | 1u << 24 | (add_lane >= 0 ? 1u : 0u) << 25;
        ++n;
    };
    const int root0 = PARC_HROT_Q_F4 + 15; // root position of the character
    const int nroot = tar_obs ? S : 0;     // the target roots take lanes 0..S-1: lane s is the shuffle source of target row 2 + s
    for (int s = 0; s < nroot; ++s) put(PARC_HROT_Q_F4 + 16 * (2 + s) + 15, root0, off_tar + s * tar_w, -1);
    put(PARC_HROT_RV_F4 + 0, PARC_HROT_RV_F4 + PARC_HROT_RV_ZERO, oc + 6, -1);
    put(PARC_HROT_RV_F4 + 1, PARC_HROT_RV_F4 + PARC_HROT_RV_ZERO, oc + 9, -1);
    for (int k = 0; k < K; ++k) {
        if (key_ids[k] < 0 || key_ids[k] >= B) return false;
        put(PARC_HROT_FK_F4 + key_ids[k], root0, off_key + 3 * k, -1);
    }
    for (int s = 0; s < nroot; ++s)
        for (int k = 0; k < K; ++k) {
            const int slot = key_slot[key_ids[k]];
            if (slot < 0 || slot >= 8) return false;
            put(PARC_HROT_FK_F4 + 32 + 8 * s + slot, PARC_HROT_Q_F4 + 16 * (2 + s) + 15, off_tar + s * tar_w + 3 + 6 * B + 3 * k, global_obs ? -1 : s);
        }
    return ok;
}
