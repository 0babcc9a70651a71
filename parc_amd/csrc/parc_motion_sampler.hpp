// parc_motion_sampler.hpp — motion-window sampler for generator training on gfx950 (parc_msamp_*, include/parc_env.h).
//
// The reference's MDMHeightfieldContactMotionSampler (mdm_heightfield_contact_motion_sampler.py) draws a batch with Python loops over
// its samples (get_hfs_from_data_helper :346, the augmentation loop :401, add_boxes_to_hf2 per box, compute_hf_mask_from_inds per frame).
// Here a batch is three launches, and every random value comes from a plan of device arrays (derived values, as parc_env_reset_with):
//   k_msamp_draw    lane per sample: fills a plan from (seed, sample index) with Philox4x32-10 (sample_motions, _sample_motion_start_times,
//                   _sample_motion_future_times, _box_hf_augmentation's and add_boxes_to_hf2's draws); lane per cell for the NOISE field
//   k_msamp_window  one wave per sample, lanes over frames x bodies: calc_motion_frame (motion_lib.py:94-126) at t0 + times[k],
//                   canonicalisation to the heading frame of the reference frame (sample_motion_data :227-249), FK with parc_char.hpp's
//                   fk_frame, lane per frame, in LDS; the target (_sample_target_info :147-161); coalesced stores from LDS
//   k_msamp_hf      one workgroup per sample: the window's cell mask as a bitset over the clip's terrain in LDS, the patch and its two
//                   bound planes in LDS (get_hfs_from_data :373-398), the augmentation (_box_hf_augmentation :293-335, maxpool_hf*
//                   terrain_util.py:1509-1535, add_boxes_to_hf2 :861-917, _noise_hf_augmentation :337-340), the clamp (:236), floor heights
// No float atomics; the only atomic is the integer OR of the LDS bitset (order-free).  Each sample is computed by its own wave /
// workgroup from its own plan entries only: its outputs are bit-identical alone or in any batch, in any position.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
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

namespace msamp {
using namespace parc;

constexpr int HF_THREADS = 256;
constexpr int GM = PARC_MSAMP_MAX_GRID;
constexpr int GP = GM + 1;                                  // odd row stride: column walks (lanes striding by Gy) hit distinct banks
// LDS of k_msamp_hf: 4 planes of 32 x 33 floats (16.5 KB, static) + the window's cell bitset (dynamic, sized for the library's largest
// terrain: 1.3 KB for 102 x 102 cells, 32 KB at the limit of PARC_MSAMP_MAX_TERRAIN_CELLS)

struct Cfg {                               // by value
    int T, ref, autoreg, zstyle, aug, Gx, Gy, nxn, nyn, maxb, max_pool, B;
    float timestep, duration, gminx, gminy, dx, max_h, box_min, box_max, pool_chance, height_chance, noise_scale, fw_min, fw_max;
    const float *times, *gridx, *gridy;    // [T], [Gx], [Gy]
};

struct Lib {                               // the resident library (ClipArrays K holds the frames and terrains)
    const MotionMeta *meta;                // [C] start = first frame, nframes, length, loop, wrap delta, fps
    const float *maxmin;                   // [cells][2]
    const long long *mask_off;             // [F + 1]
    const int *mask_cells;
    const float *cdf;                      // [C] running sum of the normalised weights
};

__device__ __forceinline__ float nanf_() { return __int_as_float(0x7fc00000); }

// root position and rotation of calc_motion_frame (motion_lib.py:94-118): lerp, slerp, the WRAP offset (:440)
__device__ __forceinline__ void root_at(const ClipArrays &K, const MotionMeta &m, float t, V3 &pos, Q4 &rot) {
    const Blend bl = frame_blend(m, t);
    const float b = bl.b, a = 1.0f - b;
    const V3 A = ld3(K.src_root_pos + 3 * (long long)bl.i0), Bv = ld3(K.src_root_pos + 3 * (long long)bl.i1);
    float x = a * A.x + b * Bv.x, y = a * A.y + b * Bv.y, z = a * A.z + b * Bv.z;
    if (m.loop == PARC_LOOP_WRAP) {
        const float ph = floorf(t / m.length);
        x = x + ph * m.dx; y = y + ph * m.dy; z = z + ph * m.dz;
    }
    pos = mk3(x, y, z);
    rot = slerp(ld4(K.src_root_rot + 4 * (long long)bl.i0), ld4(K.src_root_rot + 4 * (long long)bl.i1), b);
}

// the terrain cell under patch point (gx, gy) rotated by the heading (cos, sin) and moved to the reference root (get_hfs_from_data
// :375-380, rotate_2d_vec torch_util.py:651-662, SubTerrain.get_grid_index terrain_util.py:146-152)
__device__ __forceinline__ int patch_cell(float gx, float gy, float ch, float sh, float rx, float ry, const float *g, long long X, long long Y) {
    const float px = (gx * ch - gy * sh) + rx, py = (gx * sh + gy * ch) + ry;
    return (int)(grid_index(px, g[0], g[2], X) * Y + grid_index(py, g[1], g[3], Y));
}

// torch.clamp(x, min, max) = min(max(x, min), max); NaN in any operand gives NaN
__device__ __forceinline__ float clamp_t(float x, float mn, float mx) {
    if (x != x || mn != mn || mx != mx) return nanf_();
    return fminf(fmaxf(x, mn), mx);
}

__device__ __forceinline__ int sample_clip(const Cfg &G, const int *motion_id, int C, int enum_clip, long long s, int *status) {
    int mid = enum_clip >= 0 ? enum_clip : motion_id[s];
    if (mid < 0 || mid >= C) {
        atomicOr(status, PARC_MSAMP_STATUS_BAD_MOTION);
        mid = mid < 0 ? 0 : C - 1;
    }
    return mid;
}

struct PlanD {                             // ParcMotionSamplerPlan, writable for k_msamp_draw
    int *motion_id; float *t0, *t_future, *fnoise; int *change_height; float *height_value; int *pool_kind, *pool_size, *num_boxes;
    float *boxes, *noise;
};
struct OutD { float *root_pos, *root_rot, *joint_pos, *joint_rot, *contacts, *floor_heights, *hfs, *target_pos, *target_rot, *hf_bounds; };

// ---- window kernel ------------------------------------------------------------------------------------------------------------
// dynamic LDS per sample: jrot [T][SR] (body 0 unused), rot [T][SR], pos [T][SP], con [T][B]; SR = 4 B + 1 and SP = 3 B | 1 are odd, so
// the FK phase (lane = frame, stride SR / SP) is free of bank conflicts
__host__ __device__ __forceinline__ int win_sr(int B) { return 4 * B + 1; }
__host__ __device__ __forceinline__ int win_sp(int B) { return (3 * B) | 1; }
__host__ __device__ __forceinline__ size_t win_lds_bytes(int T, int B) { return (size_t)T * (2 * win_sr(B) + win_sp(B) + B) * sizeof(float); }

__global__ void __launch_bounds__(64) k_msamp_window(const CharTree *Mp, ClipArrays K, Lib L, Cfg G, PlanD P, OutD O, int enum_clip,
                                                     int *status) {
    extern __shared__ float s_win[];
    const CharTree &M = *Mp;
    const long long s = blockIdx.x;
    const int lane = threadIdx.x, T = G.T, B = G.B, J = B - 1;
    const int SR = win_sr(B), SP = win_sp(B);
    float *s_jrot = s_win, *s_rot = s_jrot + T * SR, *s_pos = s_rot + T * SR, *s_con = s_pos + T * SP;
    const int mid = sample_clip(G, P.motion_id, K.C, enum_clip, s, status);
    const MotionMeta meta = L.meta[mid];
    const float t0 = enum_clip >= 0 ? (float)s * G.timestep : P.t0[s];
    // the reference frame (wave-uniform)
    V3 cpos; Q4 crot;
    root_at(K, meta, t0 + G.times[G.ref], cpos, crot);
    const float heading = calc_heading(crot);
    const Q4 hinv = heading_quat_inv(heading);
    float center_h = 0.f;
    const bool floor_mode = G.zstyle == PARC_MSAMP_RELATIVE_TO_ROOT_FLOOR && O.hfs != nullptr;
    if (floor_mode) {   // hfs[num_x_neg, num_y_neg] before any shift (:386): root z is made relative to it before the canonicalisation (:238-240)
        const long long X = K.hf_dims[2 * mid], Y = K.hf_dims[2 * mid + 1];
        center_h = K.hf[K.hf_off[mid] + patch_cell(G.gridx[G.nxn], G.gridy[G.nyn], cosf(heading), sinf(heading), cpos.x, cpos.y,
                                                   K.hf_geom + 4 * mid, X, Y)];
    }
    for (int it = lane; it < T * B; it += 64) {
        const int k = it / B, j = it - k * B;
        const float t = t0 + G.times[k];
        if (j == 0) {
            V3 p; Q4 r;
            root_at(K, meta, t, p, r);
            if (floor_mode) p.z = p.z - center_h;
            p = quat_rotate(hinv, mk3(p.x - cpos.x, p.y - cpos.y, p.z - cpos.z));
            st3(s_pos + k * SP, p);
            st4(s_rot + k * SR, qmul(hinv, r));       // torch_util.quat_multiply: the written-out product
        } else {
            const Blend bl = frame_blend(meta, t);
            const float *q0 = K.src_jrot + ((long long)bl.i0 * J + (j - 1)) * 4, *q1 = K.src_jrot + ((long long)bl.i1 * J + (j - 1)) * 4;
            st4(s_jrot + k * SR + 4 * j, slerp(ld4(q0), ld4(q1), bl.b));
        }
        const Blend bl = frame_blend(meta, t);
        const float b = bl.b, a = 1.0f - b;
        s_con[k * B + j] = a * K.contacts[(long long)bl.i0 * B + j] + b * K.contacts[(long long)bl.i1 * B + j];
    }
    __syncthreads();
    for (int k = lane; k < T; k += 64)
        fk_frame(M, ld3(s_pos + k * SP), ld4(s_rot + k * SR), s_jrot + k * SR, s_pos + k * SP, s_rot + k * SR);
    if (lane == 63 && O.target_pos) {                        // _sample_target_info :147-161
        V3 fp; Q4 fr;
        root_at(K, meta, P.t_future[s], fp, fr);
        const float *nz = P.fnoise + 3 * s;
        fp = mk3(fp.x + nz[0], fp.y + nz[1], fp.z + nz[2]);
        fp = quat_rotate(hinv, mk3(fp.x - cpos.x, fp.y - cpos.y, fp.z - cpos.z));
        st3(O.target_pos + 3 * s, fp);
        *(float4 *)(O.target_rot + 4 * s) = qmul(hinv, fr);
    }
    __syncthreads();
    // stores: consecutive lanes write consecutive addresses; the quaternion outputs as one float4 per lane
    if (O.root_pos) for (int i = lane; i < T * 3; i += 64) O.root_pos[s * T * 3 + i] = s_pos[(i / 3) * SP + i % 3];
    if (O.root_rot) for (int k = lane; k < T; k += 64) *(float4 *)(O.root_rot + (s * T + k) * 4) = ld4(s_rot + k * SR);
    if (O.joint_pos) for (int i = lane; i < T * J * 3; i += 64) { const int k = i / (J * 3), r = i - k * J * 3; O.joint_pos[s * T * J * 3 + i] = s_pos[k * SP + 3 + r]; }
    if (O.joint_rot) for (int i = lane; i < T * J; i += 64) { const int k = i / J, j = i - k * J; *(float4 *)(O.joint_rot + (s * T * J + i) * 4) = ld4(s_jrot + k * SR + 4 * (j + 1)); }
    if (O.contacts) for (int i = lane; i < T * B; i += 64) O.contacts[s * T * B + i] = s_con[i];
}

// ---- heightfield kernel ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(HF_THREADS) k_msamp_hf(ClipArrays K, Lib L, Cfg G, PlanD P, OutD O, int *status) {
    __shared__ float s_hf[GM * GP], s_mx[GM * GP], s_mn[GM * GP], s_tmp[GM * GP];
    extern __shared__ unsigned s_bits[];                    // [bit_words of the launch] >= the words of every clip's terrain
    const long long s = blockIdx.x;
    const int tid = threadIdx.x, Gx = G.Gx, Gy = G.Gy, NP = Gx * Gy;
    const int mid = sample_clip(G, P.motion_id, K.C, -1, s, status);
    const MotionMeta meta = L.meta[mid];
    const float t0 = P.t0[s];
    V3 cpos; Q4 crot;
    root_at(K, meta, t0 + G.times[G.ref], cpos, crot);
    const float heading = calc_heading(crot), ch = cosf(heading), sh = sinf(heading);
    const long long X = K.hf_dims[2 * mid], Y = K.hf_dims[2 * mid + 1], cell0 = K.hf_off[mid];
    const float *g = K.hf_geom + 4 * mid;
    // 1. the window's cell mask: the stored frames round(t0 / timestep) + 0 .. T - 1, cut at the clip's end as the Python slice (:357)
    const int words = (int)((X * Y + 31) / 32);
    for (int w = tid; w < words; w += HF_THREADS) s_bits[w] = 0u;
    __syncthreads();
    {
        const long long n = meta.nframes, f0 = to_i64(rintf(t0 / G.timestep));
        const long long lo = f0 < 0 ? 0 : (f0 < n ? f0 : n), hi = f0 + G.T < lo ? lo : (f0 + G.T < n ? f0 + G.T : n);
        const long long e0 = L.mask_off[meta.start + lo], e1 = L.mask_off[meta.start + hi];
        for (long long e = e0 + tid; e < e1; e += HF_THREADS) {
            const int key = L.mask_cells[e];
            atomicOr(&s_bits[key >> 5], 1u << (key & 31));
        }
    }
    __syncthreads();
    // 2. gather the patch and its bounds
    const float def_mx = (float)((double)G.max_h * 2.0), def_mn = (float)(-(double)G.max_h * 2.0);
    for (int p = tid; p < NP; p += HF_THREADS) {
        const int ix = p / Gy, iy = p - ix * Gy;
        const int key = patch_cell(G.gridx[ix], G.gridy[iy], ch, sh, cpos.x, cpos.y, g, X, Y);
        const bool in = (s_bits[key >> 5] >> (key & 31)) & 1u;
        const int q = ix * GP + iy;
        s_hf[q] = K.hf[cell0 + key];
        s_mx[q] = in ? L.maxmin[2 * (cell0 + key)] : def_mx;
        s_mn[q] = in ? L.maxmin[2 * (cell0 + key) + 1] : def_mn;
    }
    __syncthreads();
    const float sub = G.zstyle == PARC_MSAMP_RELATIVE_TO_ROOT_FLOOR ? s_hf[G.nxn * GP + G.nyn] : cpos.z;
    __syncthreads();
    for (int p = tid; p < NP; p += HF_THREADS) {
        const int ix = p / Gy, q = ix * GP + (p - ix * Gy);
        s_hf[q] = s_hf[q] - sub; s_mx[q] = s_mx[q] - sub; s_mn[q] = s_mn[q] - sub;
        if (O.hf_bounds) { O.hf_bounds[(s * NP + p) * 2] = s_mx[q]; O.hf_bounds[(s * NP + p) * 2 + 1] = s_mn[q]; }
    }
    // 3. augmentation: every thread owns the cells p = tid + k HF_THREADS throughout; only the pools read other threads' cells
    if (G.aug == PARC_MSAMP_AUG_MAXPOOL_AND_BOXES) {
        if (P.change_height[s]) {
            const float hv = P.height_value[s];
            for (int p = tid; p < NP; p += HF_THREADS) { const int ix = p / Gy; s_hf[ix * GP + (p - ix * Gy)] = hv; }
        }
        for (int slot = 0; slot < 3; ++slot) {
            const int kind = P.pool_kind[3 * s + slot];
            int hw = P.pool_size[3 * s + slot];
            if (kind == PARC_MSAMP_POOL_NONE) continue;
            if (kind < 0 || kind > PARC_MSAMP_POOL_1D_Y || hw < 0) { if (tid == 0) atomicOr(status, PARC_MSAMP_STATUS_BAD_POOL); continue; }
            hw = hw < GM ? hw : GM;
            // max over a (2 hw + 1)-wide window, padding -inf: the 2-D pool is the x pass followed by the y pass (max is exact)
            for (int axis = 0; axis < 2; ++axis) {
                if ((axis == 0 && kind == PARC_MSAMP_POOL_1D_Y) || (axis == 1 && kind == PARC_MSAMP_POOL_1D_X)) continue;
                __syncthreads();
                for (int p = tid; p < NP; p += HF_THREADS) {
                    const int ix = p / Gy, iy = p - ix * Gy;
                    float m = s_hf[ix * GP + iy];
                    if (axis == 0) { const int a = ix - hw > 0 ? ix - hw : 0, b = ix + hw < Gx - 1 ? ix + hw : Gx - 1; for (int i = a; i <= b; ++i) m = fmaxf(m, s_hf[i * GP + iy]); }
                    else { const int a = iy - hw > 0 ? iy - hw : 0, b = iy + hw < Gy - 1 ? iy + hw : Gy - 1; for (int i = a; i <= b; ++i) m = fmaxf(m, s_hf[ix * GP + i]); }
                    s_tmp[ix * GP + iy] = m;
                }
                __syncthreads();
                for (int p = tid; p < NP; p += HF_THREADS) { const int ix = p / Gy, q = ix * GP + (p - ix * Gy); s_hf[q] = s_tmp[q]; }
            }
            for (int p = tid; p < NP; p += HF_THREADS) { const int ix = p / Gy, q = ix * GP + (p - ix * Gy); s_hf[q] = clamp_t(s_hf[q], s_mn[q], s_mx[q]); }
        }
        int nb = P.num_boxes[s];
        if (nb < 0 || nb > G.maxb) { if (tid == 0) atomicOr(status, PARC_MSAMP_STATUS_BAD_BOXES); nb = nb < 0 ? 0 : G.maxb; }
        for (int b = 0; b < nb; ++b) {                       // add_boxes_to_hf2 :881-912: a later box overwrites an earlier one
            const float *bx = P.boxes + (s * G.maxb + b) * PARC_MSAMP_BOX_FLOATS;
            const float cx = bx[0], cy = bx[1], lx = bx[2], ly = bx[3], ca = cosf(bx[4]), sa = sinf(bx[4]), h = bx[5];
            const float x1 = cx + lx / 2.f, x0 = cx - lx / 2.f, y1 = cy + ly / 2.f, y0 = cy - ly / 2.f;
            for (int p = tid; p < NP; p += HF_THREADS) {
                const int ix = p / Gy, iy = p - ix * Gy;
                const float ux = (float)ix - cx, uy = (float)iy - cy;
                const float rx = (ux * ca - uy * sa) + cx, ry = (ux * sa + uy * ca) + cy;
                if (rx < x1 && rx > x0 && ry < y1 && ry > y0) s_hf[ix * GP + iy] = h;
            }
        }
        for (int p = tid; p < NP; p += HF_THREADS) { const int ix = p / Gy, q = ix * GP + (p - ix * Gy); s_hf[q] = clamp_t(s_hf[q], s_mn[q], s_mx[q]); }
    } else if (G.aug == PARC_MSAMP_AUG_NOISE) {
        // _noise_hf_augmentation :337-340 passes the UPPER bound as clamp's min and the lower as its max: reproduced
        for (int p = tid; p < NP; p += HF_THREADS) { const int ix = p / Gy, q = ix * GP + (p - ix * Gy); s_hf[q] = clamp_t(P.noise[s * NP + p], s_mx[q], s_mn[q]); }
    }
    // 4. clamp to [-max_h, max_h] (:236) and write; floor heights from the final patch (:267-278)
    for (int p = tid; p < NP; p += HF_THREADS) {
        const int ix = p / Gy, q = ix * GP + (p - ix * Gy);
        const float v = clamp_t(s_hf[q], -G.max_h, G.max_h);
        s_hf[q] = v;
        O.hfs[s * NP + p] = v;
    }
    if (O.floor_heights) {
        __syncthreads();
        for (int k = tid; k < G.T; k += HF_THREADS) {
            const float *rp = O.root_pos + (s * G.T + k) * 3;
            const long long i = grid_index(rp[0], G.gminx, G.dx, Gx), j = grid_index(rp[1], G.gminy, G.dx, Gy);
            O.floor_heights[s * G.T + k] = s_hf[i * GP + j];
        }
    }
}

// ---- plan generator -----------------------------------------------------------------------------------------------------------------
// Philox4x32-10 keyed by the seed; counter = (sample index, block): blocks 0-4 the scalar draws, 8 + 2 b and 9 + 2 b box b.
__device__ __forceinline__ int randint_incl(float u, int m) { const int v = (int)(u * (float)(m + 1)); return v < m ? v : m; }

__global__ void k_msamp_draw(ClipArrays K, Lib L, Cfg G, PlanD P, long long n, unsigned long long seed) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    float u[4], v[4];
    philox4(seed, (unsigned long long)s, 0u, u);
    const int C = K.C;
    const float x = u[0] * L.cdf[C - 1];                      // torch.multinomial with replacement = inverse CDF per draw
    int lo = 0, hi = C - 1;
    while (lo < hi) { const int md = (lo + hi) >> 1; if (L.cdf[md] > x) hi = md; else lo = md + 1; }
    const MotionMeta m = L.meta[lo];
    P.motion_id[s] = lo;
    // _sample_motion_start_times (motion_sampler.py:39-53): rand x length for WRAP, rand x (length - sequence_duration) for CLAMP
    float t0 = 0.f;
    if (G.autoreg) t0 = m.loop == PARC_LOOP_WRAP ? u[1] * m.length : u[2] * (m.length - G.duration);
    P.t0[s] = t0;
    // _sample_motion_future_times :133-145
    const float remaining = fminf(m.length - t0, G.fw_max - G.fw_min);
    P.t_future[s] = u[3] * remaining + t0 + G.fw_min;
    philox4(seed, (unsigned long long)s, 1u, u);               // Gaussian position noise: Box-Muller on (0, 1] uniforms
    const float r0 = sqrtf(-2.f * logf(1.f - u[0])), r1 = sqrtf(-2.f * logf(1.f - u[2]));
    P.fnoise[3 * s] = G.noise_scale * (r0 * cosf(6.283185307179586f * u[1]));
    P.fnoise[3 * s + 1] = G.noise_scale * (r0 * sinf(6.283185307179586f * u[1]));
    P.fnoise[3 * s + 2] = G.noise_scale * (r1 * cosf(6.283185307179586f * u[3]));
    philox4(seed, (unsigned long long)s, 2u, u);               // _box_hf_augmentation :293-324
    philox4(seed, (unsigned long long)s, 3u, v);
    P.change_height[s] = u[0] < G.height_chance ? 1 : 0;
    P.height_value[s] = u[1] * (G.max_h - (-G.max_h)) + (-G.max_h);
    const int perm = randint_incl(v[1], 5);                   // random.shuffle of (2-D, 1-D x, 1-D y): the six orders, equally likely
    const int first = perm / 2, second = (first + 1 + (perm & 1)) % 3, third = 3 - first - second;
    const int order[3] = {first, second, third};
    const float roll[3] = {u[2], u[3], v[0]}, sz[3] = {v[2], v[3], 0.f};
    float w[4];
    philox4(seed, (unsigned long long)s, 4u, w);
    for (int k = 0; k < 3; ++k) {
        const bool use = roll[k] < G.pool_chance;
        P.pool_kind[3 * s + k] = use ? order[k] + 1 : PARC_MSAMP_POOL_NONE;
        P.pool_size[3 * s + k] = randint_incl(k < 2 ? sz[k] : w[0], G.max_pool);
    }
    const int nb = randint_incl(w[1], G.maxb);
    P.num_boxes[s] = nb;
    for (int b = 0; b < G.maxb; ++b) {                         // add_boxes_to_hf2 :883-885, :908
        philox4(seed, (unsigned long long)s, 8u + 2u * b, u);
        philox4(seed, (unsigned long long)s, 9u + 2u * b, v);
        float *bx = P.boxes + (s * G.maxb + b) * PARC_MSAMP_BOX_FLOATS;
        bx[0] = u[0] * (float)G.Gx; bx[1] = u[1] * (float)G.Gy;
        bx[2] = u[2] * (G.box_max - G.box_min) + G.box_min; bx[3] = u[3] * (G.box_max - G.box_min) + G.box_min;
        bx[4] = v[0] * 6.283185307179586f;
        bx[5] = v[1] * (G.max_h - (-G.max_h)) + (-G.max_h);
    }
}

// the NOISE field: rand_like x (max_h - min_h) + min_h, four cells per lane; counter = (1 << 40 | sample, cell / 4)
__global__ void k_msamp_draw_noise(Cfg G, float *noise, long long n, unsigned long long seed) {
    const long long NP = (long long)G.Gx * G.Gy, q = (NP + 3) / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * q) return;
    const long long s = i / q, c = i - s * q;
    float u[4];
    philox4(seed, (1ull << 40) | (unsigned long long)s, (unsigned)c, u);
    for (int k = 0; k < 4; ++k)
        if (4 * c + k < NP) noise[s * NP + 4 * c + k] = u[k] * (G.max_h - (-G.max_h)) + (-G.max_h);
}

}  // namespace msamp

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcMotionSampler : tool::CharHandle<parc::CharTree, DeviceEvents<4>> {   // mem: d_model, status, the times / grid tables of cfg
    struct Library {                      // what one parc_msamp_set_clips loads; a library is loaded when the handle holds one
        DeviceArena mem;
        ClipArrays K{};                  // the frames and terrains
        msamp::Lib L{};
        std::vector<int> clip_windows;    // num_frames - T per clip
        int bit_words = 0;                // words of the largest terrain's cell bitset
    };
    msamp::Cfg cfg{};
    std::unique_ptr<Library> lib;
    tool::StatusWords status;             // one word
    bool timed = false;
};

extern "C" void parc_msamp_destroy(ParcMotionSampler *h) { tool::destroy(h); }

extern "C" int parc_msamp_create(const ParcMotionSamplerParams *p, ParcMotionSampler **out) {
    PARC_TRY(tool::create_args("msamp", "ParcMotionSamplerParams", p, out, 2, false));
    if (p->num_frames < 1 || p->num_frames > PARC_MSAMP_MAX_FRAMES || !p->times_host)
        return fail(PARC_ERR_INVALID, "msamp: the window must have 1 .. " + std::to_string(PARC_MSAMP_MAX_FRAMES) + " frames");
    if (p->ref_frame < 0 || p->ref_frame >= p->num_frames) return fail(PARC_ERR_INVALID, "msamp: num_prev_states must be in [1, T]");
    if (p->grid_dim_x < 1 || p->grid_dim_x > PARC_MSAMP_MAX_GRID || p->grid_dim_y < 1 || p->grid_dim_y > PARC_MSAMP_MAX_GRID ||
        p->num_x_neg < 0 || p->num_x_neg >= p->grid_dim_x || p->num_y_neg < 0 || p->num_y_neg >= p->grid_dim_y || !p->grid_x_host || !p->grid_y_host)
        return fail(PARC_ERR_INVALID, "msamp: the local grid must be 1 .. " + std::to_string(PARC_MSAMP_MAX_GRID) + " points a side");
    if (p->relative_z_style != PARC_MSAMP_RELATIVE_TO_ROOT && p->relative_z_style != PARC_MSAMP_RELATIVE_TO_ROOT_FLOOR)
        return fail(PARC_ERR_INVALID, "msamp: unknown relative_z_style");
    if (p->aug_mode < PARC_MSAMP_AUG_NOISE || p->aug_mode > PARC_MSAMP_AUG_NONE) return fail(PARC_ERR_INVALID, "msamp: unknown hf_augmentation_mode");
    if (p->max_num_boxes < 0 || p->max_num_boxes > PARC_MSAMP_MAX_BOXES || p->hf_max_maxpool_size < 0)
        return fail(PARC_ERR_INVALID, "msamp: max_num_boxes must be in [0, " + std::to_string(PARC_MSAMP_MAX_BOXES) + "], hf_max_maxpool_size >= 0");
    if (!(p->timestep > 0.f) || !(p->dx > 0.f)) return fail(PARC_ERR_INVALID, "msamp: sequence_fps and horizontal_scale must be > 0");
    parc::CharTree M;
    PARC_TRY(tool::char_tree("msamp", p->model, M));
    return tool::create("msamp", p->device, M, out, [&](ParcMotionSampler &h) -> int {
        msamp::Cfg &G = h.cfg;
        G.T = p->num_frames; G.ref = p->ref_frame; G.autoreg = p->autoregressive; G.zstyle = p->relative_z_style; G.aug = p->aug_mode;
        G.Gx = p->grid_dim_x; G.Gy = p->grid_dim_y; G.nxn = p->num_x_neg; G.nyn = p->num_y_neg; G.maxb = p->max_num_boxes;
        G.max_pool = p->hf_max_maxpool_size; G.B = M.B;
        G.timestep = p->timestep; G.duration = p->sequence_duration; G.gminx = p->grid_min_x; G.gminy = p->grid_min_y; G.dx = p->dx;
        G.max_h = p->max_h; G.box_min = p->box_min_len; G.box_max = p->box_max_len; G.pool_chance = p->hf_maxpool_chance;
        G.height_chance = p->hf_change_height_chance; G.noise_scale = p->future_pos_noise_scale; G.fw_min = p->future_window_min;
        G.fw_max = p->future_window_max;
        PARC_TRY(h.status.alloc(h.mem, 1));
        PARC_TRY(h.mem.alloc(G.times, p->num_frames, p->times_host));
        PARC_TRY(h.mem.alloc(G.gridx, p->grid_dim_x, p->grid_x_host));
        return h.mem.alloc(G.gridy, p->grid_dim_y, p->grid_y_host);
    });
}

// as parc_mopt_set_clips: validate; release the old library; build the new one in a local; install it last (never a half-filled one)
extern "C" int parc_msamp_set_clips(ParcMotionSampler *h, const ParcMotionOptClips *c, const ParcMotionSamplerClipInfo *info) {
    if (!h || !c || !info) return fail(PARC_ERR_INVALID, "msamp: null argument");
    PARC_TRY(clip_batch_arrays("msamp", c));
    if (!info->hf_maxmin_host || !info->mask_off_host || !info->fps_host || !info->loop_modes_host || !info->weights_host)
        return fail(PARC_ERR_INVALID, "msamp: null clip array");
    if (info->mask_off_host[0] != 0) return fail(PARC_ERR_INVALID, "msamp: offsets must start at 0");
    const int C = c->num_clips, B = h->host_model.B, T = h->cfg.T;
    if (c->frame_off_host[C] > 0x7fffffffLL) return fail(PARC_ERR_INVALID, "msamp: at most 2^31 - 1 frames");
    std::vector<MotionMeta> meta((size_t)C);
    std::vector<float> cdf((size_t)C);
    std::vector<int> windows((size_t)C);
    int bit_words = 0;
    double wsum = 0.0;
    for (int i = 0; i < C; ++i) {
        if (!(info->weights_host[i] >= 0.0)) return fail(PARC_ERR_INVALID, "msamp: clip " + std::to_string(i) + " has a negative weight");
        wsum += info->weights_host[i];
    }
    if (!(wsum > 0.0)) return fail(PARC_ERR_INVALID, "msamp: the weights sum to 0");
    for (int i = 0; i < C; ++i) {   // before the shared per-clip checks: a clip without frames is refused as too short as well
        const long long nf = c->frame_off_host[i + 1] - c->frame_off_host[i];
        if (nf - T <= 0)   // get_motion_sequences_for_id asserts; _sample_motion_start_times would draw a negative start time
            return fail(PARC_ERR_INVALID, "msamp: clip " + std::to_string(i) + " is too short: " + std::to_string(nf) + " frames for windows of " +
                                              std::to_string(T));
    }
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("msamp", c, cb));
    const long long F = cb.F, ncell = cb.ncell;
    float run = 0.f;
    for (int i = 0; i < C; ++i) {
        const long long f0 = c->frame_off_host[i], nf = c->frame_off_host[i + 1] - f0;
        const long long X = c->hf_dims_host[2 * i], Y = c->hf_dims_host[2 * i + 1];
        if (X * Y > PARC_MSAMP_MAX_TERRAIN_CELLS)
            return fail(PARC_ERR_INVALID, "msamp: the terrain of clip " + std::to_string(i) + " has " + std::to_string(X * Y) + " cells, above the limit of " +
                                              std::to_string(PARC_MSAMP_MAX_TERRAIN_CELLS) + " (the window mask is a bitset in LDS)");
        if (info->fps_host[i] < 1) return fail(PARC_ERR_INVALID, "msamp: fps must be >= 1");
        for (long long f = f0; f < f0 + nf; ++f) {
            if (info->mask_off_host[f + 1] < info->mask_off_host[f]) return fail(PARC_ERR_INVALID, "msamp: mask offsets must not decrease");
            for (long long e = info->mask_off_host[f]; e < info->mask_off_host[f + 1]; ++e)
                if (!info->mask_cells_host || info->mask_cells_host[e] < 0 || info->mask_cells_host[e] >= X * Y)
                    return fail(PARC_ERR_INVALID, "msamp: a mask cell of clip " + std::to_string(i) + " lies outside its terrain");
        }
        MotionMeta &mm = meta[(size_t)i];
        mm.start = (int)f0; mm.nframes = (int)nf; mm.loop = info->loop_modes_host[i]; mm.fps = (float)info->fps_host[i];
        mm.length = (float)(1.0 / (double)info->fps_host[i] * (double)(nf - 1));           // motion_lib.py:313
        const float *rp = c->root_pos_host + 3 * f0;
        mm.dx = rp[3 * (nf - 1)] - rp[0]; mm.dy = rp[3 * (nf - 1) + 1] - rp[1]; mm.dz = 0.f;   // :315-316
        run += (float)(info->weights_host[i] / wsum);
        cdf[(size_t)i] = run;
        windows[(size_t)i] = (int)(nf - T);
        if ((int)((X * Y + 31) / 32) > bit_words) bit_words = (int)((X * Y + 31) / 32);
    }
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<ParcMotionSampler::Library> nl;
    PARC_TRY(tool::renew("msamp", h->lib, nl));
    ClipArrays &K = nl->K;
    msamp::Lib &L = nl->L;
    DeviceArena &mem = nl->mem;
    PARC_TRY(clip_batch_upload(mem, K, c, cb, B));
    PARC_TRY(mem.alloc(L.meta, C, meta.data()));
    PARC_TRY(mem.alloc(L.maxmin, 2 * ncell, info->hf_maxmin_host));
    PARC_TRY(mem.alloc(L.mask_off, F + 1, info->mask_off_host));
    PARC_TRY(mem.alloc(L.mask_cells, info->mask_off_host[F], info->mask_cells_host));
    PARC_TRY(mem.alloc(L.cdf, C, cdf.data()));
    nl->clip_windows.swap(windows);
    nl->bit_words = bit_words;
    h->lib = std::move(nl);
    return PARC_OK;
}

static msamp::PlanD msamp_plan(const ParcMotionSamplerPlan *p) {
    msamp::PlanD d;
    d.motion_id = (int *)p->motion_id; d.t0 = (float *)p->t0; d.t_future = (float *)p->t_future; d.fnoise = (float *)p->future_pos_noise;
    d.change_height = (int *)p->change_height; d.height_value = (float *)p->height_value; d.pool_kind = (int *)p->pool_kind;
    d.pool_size = (int *)p->pool_size; d.num_boxes = (int *)p->num_boxes; d.boxes = (float *)p->boxes; d.noise = (float *)p->noise;
    return d;
}
static msamp::OutD msamp_out(const ParcMotionSamplerOutputs *o) {
    msamp::OutD d;
    d.root_pos = o->root_pos; d.root_rot = o->root_rot; d.joint_pos = o->joint_pos; d.joint_rot = o->joint_rot; d.contacts = o->contacts;
    d.floor_heights = o->floor_heights; d.hfs = o->hfs; d.target_pos = o->target_pos; d.target_rot = o->target_rot; d.hf_bounds = o->hf_bounds;
    return d;
}

static int msamp_check_plan(ParcMotionSampler *h, const ParcMotionSamplerPlan *p, bool hf) {
    if (!h || !p) return fail(PARC_ERR_INVALID, "msamp: null argument");
    if (!h->lib) return tool::no_clips("msamp");
    if (p->n < 1) return fail(PARC_ERR_INVALID, "msamp: n must be >= 1");
    if (!p->motion_id || !p->t0 || !p->t_future || !p->future_pos_noise) return fail(PARC_ERR_INVALID, "msamp: null plan array");
    if (hf && h->cfg.aug == PARC_MSAMP_AUG_MAXPOOL_AND_BOXES &&
        (!p->change_height || !p->height_value || !p->pool_kind || !p->pool_size || !p->num_boxes || (h->cfg.maxb > 0 && !p->boxes)))
        return fail(PARC_ERR_INVALID, "msamp: MAXPOOL_AND_BOXES needs the height, pool and box arrays of the plan");
    if (hf && h->cfg.aug == PARC_MSAMP_AUG_NOISE && !p->noise) return fail(PARC_ERR_INVALID, "msamp: NOISE needs the plan's noise field");
    return PARC_OK;
}

static int msamp_launch(ParcMotionSampler *h, const ParcMotionSamplerPlan *plan, const ParcMotionSamplerOutputs *out, hipStream_t st) {
    const msamp::Cfg &G = h->cfg;
    if ((out->floor_heights && (!out->root_pos || !out->hfs)) || (out->hf_bounds && !out->hfs))
        return fail(PARC_ERR_INVALID, "msamp: floor_heights needs root_pos and hfs, hf_bounds needs hfs");
    if ((out->target_pos == nullptr) != (out->target_rot == nullptr)) return fail(PARC_ERR_INVALID, "msamp: target_pos and target_rot go together");
    const msamp::PlanD P = msamp_plan(plan);
    const msamp::OutD O = msamp_out(out);
    PARC_TRY(tool::launch(msamp::k_msamp_window, dim3((unsigned)plan->n), dim3(64), msamp::win_lds_bytes(G.T, G.B), st, h->d_model, h->lib->K, h->lib->L, G, P, O,
                       -1, h->status.d));
    HIPCHK(hipEventRecord(h->ev[2], st));
    if (out->hfs) {
        PARC_TRY(tool::launch(msamp::k_msamp_hf, dim3((unsigned)plan->n), dim3(msamp::HF_THREADS), (size_t)h->lib->bit_words * sizeof(unsigned), st, h->lib->K, h->lib->L, G, P, O,
                           h->status.d));
    }
    HIPCHK(hipEventRecord(h->ev[3], st));
    h->timed = true;
    return PARC_OK;
}

static int msamp_draw(ParcMotionSampler *h, uint64_t seed, const ParcMotionSamplerPlan *plan, hipStream_t st) {
    const msamp::Cfg &G = h->cfg;
    if (!plan->change_height || !plan->height_value || !plan->pool_kind || !plan->pool_size || !plan->num_boxes || (G.maxb > 0 && !plan->boxes))
        return fail(PARC_ERR_INVALID, "msamp: draw_plan fills every array of the plan (noise may be NULL outside NOISE mode)");
    const long long n = plan->n;
    PARC_TRY(tool::launch(msamp::k_msamp_draw, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, h->lib->K, h->lib->L, G, msamp_plan(plan), n,
                       (unsigned long long)seed));
    if (plan->noise) {
        const long long items = n * (((long long)G.Gx * G.Gy + 3) / 4);
        PARC_TRY(tool::launch(msamp::k_msamp_draw_noise, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, G, (float *)plan->noise, n,
                           (unsigned long long)seed));
    }
    return PARC_OK;
}

extern "C" int parc_msamp_sample_with(ParcMotionSampler *h, const ParcMotionSamplerPlan *plan, const ParcMotionSamplerOutputs *out, void *stream) {
    if (!out) return fail(PARC_ERR_INVALID, "msamp: null argument");
    if (int rc = msamp_check_plan(h, plan, out->hfs != nullptr)) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->ev[0], (hipStream_t)stream));
    HIPCHK(hipEventRecord(h->ev[1], (hipStream_t)stream));
    return msamp_launch(h, plan, out, (hipStream_t)stream);
}

extern "C" int parc_msamp_draw_plan(ParcMotionSampler *h, uint64_t seed, const ParcMotionSamplerPlan *plan, void *stream) {
    if (int rc = msamp_check_plan(h, plan, false)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return msamp_draw(h, seed, plan, (hipStream_t)stream);
}

extern "C" int parc_msamp_sample(ParcMotionSampler *h, uint64_t seed, const ParcMotionSamplerPlan *plan, const ParcMotionSamplerOutputs *out,
                                 void *stream) {
    if (!out) return fail(PARC_ERR_INVALID, "msamp: null argument");
    if (int rc = msamp_check_plan(h, plan, out->hfs != nullptr)) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->ev[0], (hipStream_t)stream));
    if (int rc = msamp_draw(h, seed, plan, (hipStream_t)stream)) return rc;
    HIPCHK(hipEventRecord(h->ev[1], (hipStream_t)stream));
    return msamp_launch(h, plan, out, (hipStream_t)stream);
}

extern "C" int parc_msamp_enumerate(ParcMotionSampler *h, int32_t clip, const ParcMotionSamplerOutputs *out, void *stream) {
    if (!h || !out) return fail(PARC_ERR_INVALID, "msamp: null argument");
    if (!h->lib) return tool::no_clips("msamp");
    if (clip < 0 || clip >= h->lib->K.C) return fail(PARC_ERR_INVALID, "msamp: clip out of range");
    if (out->hfs || out->floor_heights || out->target_pos || out->target_rot || out->hf_bounds)
        return fail(PARC_ERR_INVALID, "msamp: enumerate writes the motion outputs only");
    HIPCHK(hipSetDevice(h->device));
    const msamp::Cfg &G = h->cfg;
    msamp::PlanD P{};
    PARC_TRY(tool::launch(msamp::k_msamp_window, dim3((unsigned)h->lib->clip_windows[(size_t)clip]), dim3(64), msamp::win_lds_bytes(G.T, G.B),
                       (hipStream_t)stream, h->d_model, h->lib->K, h->lib->L, G, P, msamp_out(out), (int)clip, h->status.d));
    return PARC_OK;
}

extern "C" int parc_msamp_plan_status(ParcMotionSampler *h, void *stream, int32_t *status) {
    if (!h || !status) return fail(PARC_ERR_INVALID, "msamp: null argument");
    HIPCHK(hipSetDevice(h->device));
    return h->status.take(0, (hipStream_t)stream, *status);
}

extern "C" int parc_msamp_kernel_times(ParcMotionSampler *h, float *ms3) {
    if (!h || !ms3) return fail(PARC_ERR_INVALID, "msamp: null argument");
    const tool::Span spans[] = {{h->timed, 0, 1}, {h->timed, 1, 2}, {h->timed, 2, 3}};   // draw, window, hf
    return tool::span_times("msamp: nothing sampled yet", h->device, h->ev, spans, ms3);
}
