// parc_motion_terrain.hpp — motion-terrain analysis on gfx950 (parc_mterr_*, include/parc_env.h).
//
// One geometric pass serves three places of the reference: the dataset preprocessing of terrain_util.compute_hf_extra_vals
// (terrain_util.py:1851-1947: per-frame cell masks, the lowest body point per cell, the augmentation bounds hf_maxmin), the clip
// scores of mdm_path.compute_motion_loss (mdm_path.py:31-127: penetration and contact against the exact column-box SDF of the whole
// terrain) and the jerk statistics of scripts/motion_tests/compute_losses.py:163-174.  All clips of a batch go through:
//   k_mterr_fk      lane per frame: validity of the frame's inputs, FK (parc_char.hpp's fk_frame) into a per-frame workspace
//   k_mterr_init    lane per cell:  lowest point = 99999.9999f (encoded), touched = 0
//   k_mterr_points  block per frame, lane per sample point: world point, cell index (round half to even of a true division, clamped),
//                   integer atomicMin of the encoded height + touched flag, exact ground / air SDF (ring-pruned or brute force);
//                   a bitonic sort of the frame's cell keys in LDS, duplicates dropped and compacted with a wave-ballot scan;
//                   lane b < B: the body's penetration sum, contact term and jerk window; lane 0: the frame's partial sums
//   k_mterr_reduce  lane per clip: the per-frame partial sums in frame order (double accumulator), max root z, jerk statistics
//   k_mterr_cells   lane per cell: hf_maxmin in compute_hf_extra_vals' order (defaults, masked cells, jump cells)
//   k_mterr_gather  block per frame: the frame's unique cells to their place in the [K][2] output (offsets from the host's scan)
// No float atomics and no reduction whose order depends on the batch: a clip's results are bit-identical alone or in any batch.
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

namespace mterr {
using namespace parc;

constexpr int PT_THREADS = 256;
constexpr int MAXP = PARC_MOPT_MAX_POINTS;
constexpr int MAXB = PARC_MAX_BODIES;
constexpr int NOUT = PARC_MTERR_CLIP_OUTPUTS;
enum { S_PEN = 0, S_CONTACT, S_JERK_SUM, S_JERK_CNT, S_ROOT_Z, NS };
enum { O_PEN = 0, O_CONTACT, O_MEAN_JERK, O_JERK_FRAC, O_MAX_ROOT_Z, O_MIN_HF };
constexpr int KEY_NONE = 0x7fffffff;   // sorts after every cell key (keys are < X * Y <= INT32_MAX)

struct Cfg {                           // by value
    int sdf_mode, sort_n;              // sort_n: the smallest power of two >= the number of points
    float jump_buf, max_jerk;
    double z_buf;
};

struct Work {
    float *pos, *rot;                  // [F][B][3], [F][B][4]
    int *valid;                        // [F] inputs finite
    float *fterms;                     // [F][NS]
    int *keys;                         // [F][P]: the frame's unique cell keys i * Y + j, ascending, first cnt[f] used
    int *cnt;                          // [F]
    long long *ind_off;                // [F] exclusive scan of cnt (host)
    int *minh;                         // [cells] order-preserving integer encoding of the lowest body point
    int *touched;                      // [cells]
    float *maxmin;                     // [cells][2]
    float *clip_out;                   // [C][NOUT]
};

// order-preserving float <-> int (for integer atomicMin): non-negative floats keep their bits, negative ones flip the magnitude bits
__device__ __forceinline__ int enc_f(float v) { const int i = __float_as_int(v); return i >= 0 ? i : i ^ 0x7fffffff; }
__host__ __device__ __forceinline__ float dec_f(int e) {
    const int i = e >= 0 ? e : e ^ 0x7fffffff;
    float v;
    memcpy(&v, &i, sizeof(v));
    return v;
}

__device__ __forceinline__ bool fin3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// the ground box [base_z, h] and the air box [h, top_z] of one cell (points_hf_sdf, terrain_util.py:1736-1794; sdBox geom_util.py:124)
__device__ __forceinline__ float ground_sd(V3 x, float cx, float cy, float hx, float hy, float h, float base_z) {
    return sd_box(mk3(x.x - cx, x.y - cy, x.z - (h + base_z) / 2.f), mk3(hx, hy, (h - base_z) / 2.f));
}
__device__ __forceinline__ float air_sd(V3 x, float cx, float cy, float hx, float hy, float h, float top_z) {
    return sd_box(mk3(x.x - cx, x.y - cy, x.z - (h + top_z) / 2.f), mk3(hx, hy, (top_z - h) / 2.f));
}

// points_hf_sdf's cell centres: torch.linspace(0, (n - 1) dx, n) + min.  The CPU kernel computes step * i below the middle and
// end - step * (n - 1 - i) with one rounding above it (the vectorised fused multiply-add); end = (n - 1) dx in double, then fp32.
struct Axis {
    float mn, end, step;
    long long n;
};
__device__ __forceinline__ Axis make_axis(float mn, float d, long long n) {
    Axis a;
    a.mn = mn; a.n = n;
    a.end = (float)((double)(n - 1) * (double)d);
    a.step = n > 1 ? a.end / (float)(n - 1) : 0.f;
    return a;
}
__device__ __forceinline__ float centre(const Axis &a, long long i) {
    return (i < a.n / 2 ? a.step * (float)i : fmaf(-a.step, (float)(a.n - 1 - i), a.end)) + a.mn;
}

// Exact minimum of the ground and the air box SDF over the WHOLE terrain.  Brute force: every cell.  Pruned: Chebyshev rings around
// the point's (clamped) cell c; every cell of ring r >= 1 is at least min(r dx - |x - cx_c| - dx/2, r dy - |y - cy_c| - dy/2) away from
// the point in xy, and a box the point lies outside of in xy has an SDF >= that distance.  A minimum stops being searched once the bound,
// less a margin, exceeds it (and 0): no skipped cell can reach it, so both modes return the same bits.  The margin, 1e-5 x (1 + |x| +
// |y| + |min x| + |min y| + r max(dx, dy)), is about 80 fp32 ulps of the largest coordinate involved: it covers the rounding of the
// linspace centres (<= 2 ulps of |min| + i dx, i <= the point's cell + r), of the bound itself and of the cell SDFs.
// Cells outside the grid do not exist (rings are clipped).
// The heights come through `H`: hf.row(i)[j] is the height of cell (i, j).  HfContig is the clip's own [X][Y] array; the path selection
// (parc_mpath_select.hpp) reads a slice of a terrain through two index tables.
struct HfContig {
    const float *hf;
    long long Y;
    __device__ __forceinline__ const float *row(long long i) const { return hf + i * Y; }
};
template <typename H>
__device__ __forceinline__ void terrain_sdf(V3 x, const H &hf, long long X, long long Y, float mnx, float mny, float dx, float dy,
                                            float base_z, int brute, float &out_g, float &out_a) {
    const float hx = dx / 2.f, hy = dy / 2.f, top_z = -base_z;
    const Axis ax = make_axis(mnx, dx, X), ay = make_axis(mny, dy, Y);
    float bg = INFINITY, ba = INFINITY;
    if (brute) {
        for (long long i = 0; i < X; ++i) {
            const float cx = centre(ax, i);
            const auto row = hf.row(i);
            for (long long j = 0; j < Y; ++j) {
                const float cy = centre(ay, j), h = row[j];
                bg = fminf(bg, ground_sd(x, cx, cy, hx, hy, h, base_z));
                ba = fminf(ba, air_sd(x, cx, cy, hx, hy, h, top_z));
            }
        }
        out_g = bg; out_a = ba;
        return;
    }
    const long long ci = grid_index(x.x, mnx, dx, X), cj = grid_index(x.y, mny, dy, Y);
    const float ex = fabsf(x.x - centre(ax, ci)), ey = fabsf(x.y - centre(ay, cj));
    const float margin0 = 1e-5f * (1.f + fabsf(x.x) + fabsf(x.y) + fabsf(mnx) + fabsf(mny)), dmax = fmaxf(dx, dy);
    long long rmax = ci > X - 1 - ci ? ci : X - 1 - ci;
    rmax = rmax > cj ? rmax : cj;
    rmax = rmax > Y - 1 - cj ? rmax : Y - 1 - cj;
    bool need_g = true, need_a = true;
    for (long long r = 0; r <= rmax; ++r) {
        if (r > 0) {
            const float lb = fminf((float)r * dx - ex - hx, (float)r * dy - ey - hy) - (margin0 + 1e-5f * ((float)r * dmax));
            need_g = need_g && !(lb > fmaxf(bg, 0.f));
            need_a = need_a && !(lb > fmaxf(ba, 0.f));
            if (!need_g && !need_a) break;
        }
        const long long i0 = ci - r > 0 ? ci - r : 0, i1 = ci + r < X - 1 ? ci + r : X - 1;
        for (long long i = i0; i <= i1; ++i) {
            // the ring's first and last rows: every column in [cj - r, cj + r]; the rows between: its two end columns only
            const bool edge_row = (i == ci - r) || (i == ci + r);
            const long long ja = edge_row ? (cj - r > 0 ? cj - r : 0) : cj - r;
            const long long jb = edge_row ? (cj + r < Y - 1 ? cj + r : Y - 1) : cj + r;
            const long long step = edge_row ? 1 : 2 * r;
            const float cx = centre(ax, i);
            const auto row = hf.row(i);
            for (long long j = ja; j <= jb; j += step) {
                if (j < 0 || j >= Y) continue;
                const float cy = centre(ay, j), h = row[j];
                if (need_g) bg = fminf(bg, ground_sd(x, cx, cy, hx, hy, h, base_z));
                if (need_a) ba = fminf(ba, air_sd(x, cx, cy, hx, hy, h, top_z));
            }
        }
    }
    out_g = bg; out_a = ba;
}
__device__ __forceinline__ void terrain_sdf(V3 x, const float *hf, long long X, long long Y, float mnx, float mny, float dx, float dy,
                                            float base_z, int brute, float &out_g, float &out_a) {
    terrain_sdf(x, HfContig{hf, Y}, X, Y, mnx, mny, dx, dy, base_z, brute, out_g, out_a);
}

// compute_motion_loss: base_z = torch.min(hf).item() - 10.0 (a Python float), used by fp32 tensor ops
__device__ __forceinline__ float clip_base_z(const FrameClips &K, int c) { return (float)((double)K.hf_min[c] - 10.0); }

// ---- kernels ----------------------------------------------------------------------------------------------------------------
__global__ void k_mterr_fk(const CharPoints *Mp, FrameClips K, Work W) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= K.F) return;
    const CharPoints &M = *Mp;
    const int B = M.B;
    const V3 rp = ld3(K.src_root_pos + 3 * f);
    const Q4 rq = ld4(K.src_root_rot + 4 * f);
    bool ok = fin3(rp) && fin3(mk3(rq.x, rq.y, rq.z)) && isfinite(rq.w);
    const float *jr = K.src_jrot + f * (B - 1) * 4;          // [B-1][4]: joint j's rotation at jr + 4 (j - 1)
    for (int k = 0; k < (B - 1) * 4; ++k) ok = ok && isfinite(jr[k]);
    for (int b = 0; b < B; ++b) ok = ok && isfinite(K.contacts[f * B + b]);
    // fk_frame reads joint j's rotation at base + 4 j for j >= 1 only
    fk_frame(M, rp, rq, jr - 4, W.pos + f * B * 3, W.rot + f * B * 4);
    W.valid[f] = ok ? 1 : 0;
}

__global__ void k_mterr_init(long long ncell, Work W) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncell) return;
    W.minh[i] = enc_f(99999.9999f);
    W.touched[i] = 0;
}

__global__ void __launch_bounds__(PT_THREADS) k_mterr_points(const CharPoints *Mp, FrameClips K, Work W, Cfg G) {
    __shared__ float s_x[MAXP][3], s_c[MAXP], s_pen[MAXP];
    __shared__ int s_key[MAXP];
    __shared__ float s_body[MAXB][4];
    __shared__ int s_bad, s_wave[PT_THREADS / 64];
    const long long f = blockIdx.x;
    const CharPoints &M = *Mp;
    const int B = M.B, P = M.P, tid = threadIdx.x;
    const int c = K.frame_clip[f];
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1], cell0 = K.hf_off[c];
    const float *g = K.hf_geom + 4 * c;
    const float *hf = K.hf + cell0;
    const float base_z = clip_base_z(K, c);
    const float *pos = W.pos + f * B * 3, *rot = W.rot + f * B * 4;
    if (tid == 0) s_bad = W.valid[f] ? 0 : 1;
    __syncthreads();
    for (int k = tid; k < P; k += PT_THREADS) {
        const int b = M.pt_body[k];
        const V3 x = add3(quat_rotate(ld4(rot + 4 * b), mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2])), ld3(pos + 3 * b));
        s_x[k][0] = x.x; s_x[k][1] = x.y; s_x[k][2] = x.z;
        if (!fin3(x)) s_bad = 1;
    }
    __syncthreads();
    const bool ok = s_bad == 0;
    for (int k = tid; k < G.sort_n; k += PT_THREADS) {
        int key = KEY_NONE;
        float cl = 0.f, pen = 0.f;
        if (k < P && ok) {
            const V3 x = mk3(s_x[k][0], s_x[k][1], s_x[k][2]);
            const long long i = grid_index(x.x, g[0], g[2], X), j = grid_index(x.y, g[1], g[3], Y);
            key = (int)(i * Y + j);
            atomicMin(W.minh + cell0 + key, enc_f(x.z));
            W.touched[cell0 + key] = 1;
            float sg, sa;
            terrain_sdf(x, hf, X, Y, g[0], g[1], g[2], g[3], base_z, G.sdf_mode, sg, sa);
            cl = fmaxf(sg, 0.f);                              // clamp(positive_sdfs, min=0)
            pen = fmaxf(sa, 0.f);                             // -clamp(-air, max=0)
        }
        s_key[k] = key;
        if (k < P) { s_c[k] = cl; s_pen[k] = pen; }
    }
    __syncthreads();
    // bitonic sort of the keys (ascending = torch.unique(dim=0)'s lexicographic (i, j) order)
    for (int size = 2; size <= G.sort_n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < G.sort_n; i += PT_THREADS) {
                const int l = i ^ stride;
                if (l > i) {
                    const int a = s_key[i], b = s_key[l];
                    if ((a > b) == ((i & size) == 0)) { s_key[i] = b; s_key[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    // drop duplicates, compact in order: per chunk of PT_THREADS keys a wave ballot + the wave totals
    int base = 0;
    const int lane = tid & 63, wave = tid >> 6;
    for (int k0 = 0; k0 < G.sort_n; k0 += PT_THREADS) {
        const int k = k0 + tid;
        const bool first = k < G.sort_n && s_key[k] != KEY_NONE && (k == 0 || s_key[k] != s_key[k - 1]);
        const unsigned long long m = __ballot(first);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = base, tot = base;
        for (int w = 0; w < PT_THREADS / 64; ++w) { off += w < wave ? s_wave[w] : 0; tot += s_wave[w]; }
        if (first) W.keys[f * P + off + __popcll(m & ((1ull << lane) - 1ull))] = s_key[k];
        __syncthreads();
        base = tot;
    }
    // per body: penetration sum, contact term (min over the body's points of the clamped ground SDF x the contact flag), jerk window
    const long long fl = f - K.frame_off[c], n = K.frame_off[c + 1] - K.frame_off[c];
    if (tid < B) {
        const int b = tid, k0 = M.pt_start[b], np = M.pt_count[b];
        float pen = 0.f, best = INFINITY;
        for (int k = k0; k < k0 + np; ++k) { pen += s_pen[k]; best = fminf(best, s_c[k]); }
        const int cid = M.contact_id[b];
        const float con = (cid >= 0 && np > 0) ? best * K.contacts[f * B + cid] : 0.f;
        float jm = 0.f, jc = 0.f;
        if (fl + 3 < n) {                                    // compute_losses.py:163-174 in its operation order, dt = 1/30 in fp32
            const float dt = (float)(1.0 / 30.0);
            V3 p[4], v[3], a[2];
            for (int t = 0; t < 4; ++t) p[t] = ld3(W.pos + ((f + t) * B + b) * 3);
            for (int t = 0; t < 3; ++t) v[t] = mk3((p[t + 1].x - p[t].x) / dt, (p[t + 1].y - p[t].y) / dt, (p[t + 1].z - p[t].z) / dt);
            for (int t = 0; t < 2; ++t) a[t] = mk3((v[t + 1].x - v[t].x) / dt, (v[t + 1].y - v[t].y) / dt, (v[t + 1].z - v[t].z) / dt);
            const V3 j = mk3((a[1].x - a[0].x) / dt, (a[1].y - a[0].y) / dt, (a[1].z - a[0].z) / dt);
            jm = norm3(j);
            jc = jm > G.max_jerk ? 1.f : 0.f;
        }
        s_body[b][0] = pen; s_body[b][1] = con; s_body[b][2] = jm; s_body[b][3] = jc;
    }
    __syncthreads();
    if (tid == 0) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) for (int q = 0; q < 4; ++q) t[q] += s_body[b][q];
        float *o = W.fterms + f * NS;
        const float nan = __int_as_float(0x7fc00000);
        o[S_PEN] = ok ? t[0] : nan; o[S_CONTACT] = ok ? t[1] : nan;
        o[S_JERK_SUM] = ok ? t[2] : nan; o[S_JERK_CNT] = ok ? t[3] : nan;
        o[S_ROOT_Z] = ok ? pos[2] : nan;
        W.cnt[f] = ok ? base : 0;
    }
}

__global__ void k_mterr_reduce(FrameClips K, Work W, int B) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K.C) return;
    double pen = 0.0, con = 0.0, js = 0.0, jc = 0.0;
    float mz = -INFINITY;
    bool nan_z = false;
    for (long long f = K.frame_off[c]; f < K.frame_off[c + 1]; ++f) {
        const float *t = W.fterms + f * NS;
        pen += (double)t[S_PEN]; con += (double)t[S_CONTACT]; js += (double)t[S_JERK_SUM]; jc += (double)t[S_JERK_CNT];
        const float z = t[S_ROOT_Z];
        if (!(z == z)) nan_z = true; else mz = fmaxf(mz, z);  // torch.max propagates NaN
    }
    const long long n = K.frame_off[c + 1] - K.frame_off[c];
    const float nan = __int_as_float(0x7fc00000);
    float *o = W.clip_out + (long long)c * NOUT;
    o[O_PEN] = (float)pen;
    o[O_CONTACT] = (float)con;
    // mean over the (n - 3) x B jerk magnitudes; the count of those above max_jerk divided by n - 3 (frames, not samples: the reference's
    // quirk, so the fraction can exceed 1)
    o[O_MEAN_JERK] = n >= 4 ? (float)(js / ((double)(n - 3) * (double)B)) : nan;
    o[O_JERK_FRAC] = n >= 4 ? (float)(jc / (double)(n - 3)) : nan;
    o[O_MAX_ROOT_Z] = nan_z ? nan : mz;
    o[O_MIN_HF] = K.hf_min[c];
}

// compute_hf_extra_vals (terrain_util.py:1920-1945): Python-float sums in double rounded to fp32, the jump test and bound in fp32
__global__ void k_mterr_cells(FrameClips K, Work W, Cfg G, long long ncell) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncell) return;
    int lo = 0, hi = K.C - 1;                                 // the clip whose cells hold i (hf_off strictly increasing)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (K.hf_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const float h = K.hf[i], mz = W.clip_out[(long long)lo * NOUT + O_MAX_ROOT_Z];
    const float low = (float)((double)K.hf_min[lo] - G.z_buf);
    float mx = (float)((double)mz + G.z_buf), mn = low;
    if (W.touched[i]) {
        mx = h; mn = h;
        const float mbh = dec_f(W.minh[i]);
        if (mbh - h >= G.jump_buf) { mx = mbh - G.jump_buf; mn = low; }
    }
    W.maxmin[2 * i] = mx;
    W.maxmin[2 * i + 1] = mn;
}

__global__ void k_mterr_gather(FrameClips K, Work W, int P, int *out) {
    const long long f = blockIdx.x;
    const int c = K.frame_clip[f];
    const int Y = K.hf_dims[2 * c + 1], n = W.cnt[f];
    const long long o = W.ind_off[f];
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int key = W.keys[f * P + k];
        out[2 * (o + k)] = key / Y;
        out[2 * (o + k) + 1] = key % Y;
    }
}

// test entry: the raw ground / air SDF minima of every sample point of frames [f0, f0 + gridDim.x)
__global__ void __launch_bounds__(PT_THREADS) k_mterr_point_sdf(const CharPoints *Mp, FrameClips K, Work W, Cfg G, long long f0,
                                                                 float *ground, float *air) {
    const long long fi = blockIdx.x, f = f0 + fi;
    const CharPoints &M = *Mp;
    const int B = M.B, P = M.P;
    const int c = K.frame_clip[f];
    const long long X = K.hf_dims[2 * c], Y = K.hf_dims[2 * c + 1];
    const float *g = K.hf_geom + 4 * c;
    const float *pos = W.pos + f * B * 3, *rot = W.rot + f * B * 4;
    for (int k = threadIdx.x; k < P; k += PT_THREADS) {
        const int b = M.pt_body[k];
        const V3 x = add3(quat_rotate(ld4(rot + 4 * b), mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2])), ld3(pos + 3 * b));
        float sg, sa;
        terrain_sdf(x, K.hf + K.hf_off[c], X, Y, g[0], g[1], g[2], g[3], clip_base_z(K, c), G.sdf_mode, sg, sa);
        ground[fi * P + k] = sg;
        air[fi * P + k] = sa;
    }
}

}  // namespace mterr

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcMotionTerrain : tool::CharHandle<parc::CharPoints, DeviceEvents<8>> {   // mem: d_model
    struct Batch {                        // what one parc_mterr_set_clips loads; a batch is loaded when the handle holds one
        DeviceArena mem;
        FrameClips K{};
        mterr::Work W{};
        std::vector<int> counts;          // per-frame mask counts of the last run
        std::vector<long long> offsets;
        long long F = 0, ncell = 0, total = 0;
        bool ran = false;
    };
    mterr::Cfg cfg{};
    std::unique_ptr<Batch> batch;
    DeviceArena inds;                     // d_inds alone: released and allocated anew when it must grow
    int *d_inds = nullptr;                // [inds_cap][2]: parc_mterr_get_mask_inds' output
    long long inds_cap = 0;
    float kernel_ms[6] = {};
};

extern "C" void parc_mterr_destroy(ParcMotionTerrain *h) { tool::destroy(h); }

extern "C" int parc_mterr_create(const ParcMotionTerrainParams *p, ParcMotionTerrain **out) {
    PARC_TRY(tool::create_args("mterr", "ParcMotionTerrainParams", p, out, 1, true));
    if (p->num_points < 1 || p->num_points > PARC_MOPT_MAX_POINTS || !p->points_host || !p->point_body_host)
        return fail(PARC_ERR_INVALID, "mterr: num_points must be in [1, 512] with points and point bodies given");
    if (p->sdf_mode != PARC_MTERR_SDF_PRUNED && p->sdf_mode != PARC_MTERR_SDF_BRUTE) return fail(PARC_ERR_INVALID, "mterr: unknown sdf_mode");
    parc::CharPoints M;
    PARC_TRY(tool::char_tree("mterr", p->model, M));
    PARC_TRY(model_points("mterr", M, p->num_points, p->points_host, p->point_body_host, p->contact_body_id));
    int sort_n = 1;
    while (sort_n < M.P) sort_n <<= 1;
    return tool::create("mterr", p->device, M, out, [&](ParcMotionTerrain &h) -> int {
        h.cfg.sdf_mode = p->sdf_mode; h.cfg.sort_n = sort_n;
        h.cfg.z_buf = p->z_buf; h.cfg.jump_buf = (float)p->jump_buf; h.cfg.max_jerk = (float)p->max_jerk;
        return PARC_OK;
    });
}

// as parc_mopt_set_clips: validate; release the old batch; build the new one in a local; install it last
extern "C" int parc_mterr_set_clips(ParcMotionTerrain *h, const ParcMotionOptClips *c) {
    if (!h || !c) return fail(PARC_ERR_INVALID, "mterr: null argument");
    PARC_TRY(clip_batch_arrays("mterr", c));
    for (int i = 0; i < c->num_clips; ++i) {   // the cell-count bound (a cell index is an int in the kernels), under the analyser's own wording
        const long long X = c->hf_dims_host[2 * i], Y = c->hf_dims_host[2 * i + 1];
        if (X < 1 || Y < 1 || X * Y > 0x7fffffffLL || c->hf_off_host[i + 1] - c->hf_off_host[i] != X * Y)
            return fail(PARC_ERR_INVALID, "mterr: heightfield dims / offsets disagree (dims >= 1, at most 2^31 - 1 cells)");
    }
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("mterr", c, cb));
    const int C = cb.C, B = h->host_model.B, P = h->host_model.P;
    const long long F = cb.F, ncell = cb.ncell;
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<ParcMotionTerrain::Batch> nb;
    PARC_TRY(tool::renew("mterr", h->batch, nb));
    FrameClips &K = nb->K;
    mterr::Work &W = nb->W;
    DeviceArena &mem = nb->mem;
    PARC_TRY(clip_batch_upload(mem, K, c, cb, B));
    PARC_TRY(clip_batch_upload_frames(mem, K, cb));
    PARC_TRY(mem.alloc(W.pos, 3 * F * B));
    PARC_TRY(mem.alloc(W.rot, 4 * F * B));
    PARC_TRY(mem.alloc(W.valid, F));
    PARC_TRY(mem.alloc(W.fterms, F * mterr::NS));
    PARC_TRY(mem.alloc(W.keys, F * P));
    PARC_TRY(mem.alloc(W.cnt, F));
    PARC_TRY(mem.alloc(W.ind_off, F));
    PARC_TRY(mem.alloc(W.minh, ncell));
    PARC_TRY(mem.alloc(W.touched, ncell));
    PARC_TRY(mem.alloc(W.maxmin, 2 * ncell));
    PARC_TRY(mem.alloc(W.clip_out, (long long)C * mterr::NOUT));
    nb->F = F; nb->ncell = ncell;
    nb->counts.assign((size_t)F, 0);
    nb->offsets.assign((size_t)F, 0);
    h->batch = std::move(nb);
    return PARC_OK;
}

extern "C" int parc_mterr_run(ParcMotionTerrain *h, float *clip_out, int32_t *mask_counts, float *hf_maxmin, int64_t *total_inds) {
    PARC_TRY(tool::check_loaded("mterr", h, &ParcMotionTerrain::batch));
    ParcMotionTerrain::Batch &b = *h->batch;
    HIPCHK(hipSetDevice(h->device));
    const long long F = b.F, ncell = b.ncell;
    const int C = b.K.C;
    HIPCHK(hipEventRecord(h->ev[0], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_fk, dim3(blocks(F, 64)), dim3(64), 0, 0, h->d_model, b.K, b.W));
    HIPCHK(hipEventRecord(h->ev[1], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_init, dim3(blocks(ncell, 256)), dim3(256), 0, 0, ncell, b.W));
    HIPCHK(hipEventRecord(h->ev[2], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_points, dim3((unsigned)F), dim3(mterr::PT_THREADS), 0, 0, h->d_model, b.K, b.W, h->cfg));
    HIPCHK(hipEventRecord(h->ev[3], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_reduce, dim3(blocks(C, 64)), dim3(64), 0, 0, b.K, b.W, h->host_model.B));
    HIPCHK(hipEventRecord(h->ev[4], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_cells, dim3(blocks(ncell, 256)), dim3(256), 0, 0, b.K, b.W, h->cfg, ncell));
    HIPCHK(hipEventRecord(h->ev[5], 0));
    HIPCHK(hipMemcpy(b.counts.data(), b.W.cnt, (size_t)F * sizeof(int), hipMemcpyDeviceToHost));
    long long tot = 0;                                        // exclusive scan of the per-frame counts, in frame order
    for (long long f = 0; f < F; ++f) { b.offsets[f] = tot; tot += b.counts[f]; }
    HIPCHK(hipMemcpy(b.W.ind_off, b.offsets.data(), (size_t)F * sizeof(long long), hipMemcpyHostToDevice));
    for (int k = 0; k < 5; ++k) PARC_TRY(h->ev.elapsed(h->kernel_ms[k], k, k + 1));
    b.total = tot;
    b.ran = true;
    if (clip_out) HIPCHK(hipMemcpy(clip_out, b.W.clip_out, (size_t)C * mterr::NOUT * sizeof(float), hipMemcpyDeviceToHost));
    if (mask_counts) memcpy(mask_counts, b.counts.data(), (size_t)F * sizeof(int));
    if (hf_maxmin) HIPCHK(hipMemcpy(hf_maxmin, b.W.maxmin, (size_t)ncell * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (total_inds) *total_inds = tot;
    return PARC_OK;
}

extern "C" int parc_mterr_get_mask_inds(ParcMotionTerrain *h, int32_t *inds) {
    PARC_TRY(tool::check_ran("mterr", h, &ParcMotionTerrain::batch));
    const ParcMotionTerrain::Batch &b = *h->batch;
    if (!inds && b.total > 0) return fail(PARC_ERR_INVALID, "mterr: null output");
    h->kernel_ms[5] = 0.f;
    if (b.total == 0) return PARC_OK;
    HIPCHK(hipSetDevice(h->device));
    if (b.total > h->inds_cap) {
        h->inds.release();
        h->d_inds = nullptr; h->inds_cap = 0;   // a failed allocation leaves no buffer, not a stale one
        PARC_TRY(h->inds.alloc(h->d_inds, 2 * b.total));
        h->inds_cap = b.total;
    }
    HIPCHK(hipEventRecord(h->ev[6], 0));
    PARC_TRY(tool::launch(mterr::k_mterr_gather, dim3((unsigned)b.F), dim3(256), 0, 0, b.K, b.W, h->host_model.P, h->d_inds));
    HIPCHK(hipEventRecord(h->ev[7], 0));
    HIPCHK(hipMemcpy(inds, h->d_inds, (size_t)b.total * 2 * sizeof(int), hipMemcpyDeviceToHost));
    return h->ev.elapsed(h->kernel_ms[5], 6, 7);
}

extern "C" int parc_mterr_get_min_heights(ParcMotionTerrain *h, float *min_heights, int32_t *touched) {
    PARC_TRY(tool::check_ran("mterr", h, &ParcMotionTerrain::batch));
    HIPCHK(hipSetDevice(h->device));
    const mterr::Work &W = h->batch->W;
    const size_t n = (size_t)h->batch->ncell;
    if (min_heights) {
        std::vector<int> e(n);
        HIPCHK(hipMemcpy(e.data(), W.minh, n * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) min_heights[i] = mterr::dec_f(e[i]);
    }
    if (touched) HIPCHK(hipMemcpy(touched, W.touched, n * sizeof(int), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_mterr_point_sdf(ParcMotionTerrain *h, int64_t frame0, int32_t num_frames, float *ground, float *air) {
    PARC_TRY(tool::check_ran("mterr", h, &ParcMotionTerrain::batch));
    const ParcMotionTerrain::Batch &b = *h->batch;
    if (num_frames < 1 || frame0 < 0 || frame0 + num_frames > b.F || !ground || !air) return fail(PARC_ERR_INVALID, "mterr: bad point_sdf range");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)num_frames * h->host_model.P;
    DeviceArena tmp;                      // this call's output
    float *d = nullptr;
    PARC_TRY(tmp.alloc(d, 2 * (long long)n));
    PARC_TRY(tool::launch(mterr::k_mterr_point_sdf, dim3((unsigned)num_frames), dim3(mterr::PT_THREADS), 0, 0, h->d_model, b.K, b.W, h->cfg,
                       (long long)frame0, d, d + n));
    HIPCHK(hipMemcpy(ground, d, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(air, d + n, n * sizeof(float), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_mterr_kernel_times(ParcMotionTerrain *h, float *ms6) {
    return tool::stored_times("mterr", h, &ParcMotionTerrain::kernel_ms, ms6);
}
