// parc_motion_aug.hpp — batched motion-terrain augmenter on gfx950 (parc_maug_*, include/parc_env.h).
//
// The reference grows a hand-made dataset one motion at a time (scripts/run_simple_augment_motions.py:144-202): cut a window of a source
// clip, turn it about the origin, stretch x and y, pad the terrain and slice it around the motion (terrain_util.pad :236,
// slice_terrain_around_motion :1587), re-anchor both at frame 0, then scale the heights or drop rotated boxes under frames of the motion
// (add_boxes_to_hf_at_xy_points :930).  Stage 2 saves a mirrored copy beside every optimised motion (parc_2_kin_gen.py:490-510:
// motion_edit_lib.flip_motion_about_XZ_plane :343, SubTerrain.flip_by_XZ_axis :182).  Here n variations are one run of short launches,
// and every random value comes from a plan of device arrays (derived values, as 8f / 8h):
//   k_maug_layout   lane per variation: the (clamped) frame count; k_maug_scan turns the counts into output offsets
//   k_maug_frames   one wave per variation, lanes stride the frames of the window: heading, scale, the wave-wide min / max of x and y
//                   (xor shuffles), the slice bounds and point counts, canon_xy / canon_z, the localised (and mirrored) frames
//   k_maug_terrain  one wave (every slice of the launch <= WAVE_CELLS cells) or one workgroup of 256 per variation, lanes stride the cells:
//                   the gather through get_grid_index on the padded terrain, - canon_z, the edit (boxes staged in LDS, 576 B), the mirror
// Every kernel is a template on DRAW: false reads the plan, true draws the same values in place with the functions k_maug_draw uses, so
// parc_maug_augment gives the bits of parc_maug_draw_plan + parc_maug_augment_with.  No atomics except the integer OR of the status word.
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

namespace maug {
using namespace parc;

constexpr int MAXB = PARC_MAUG_MAX_BOXES, BF = PARC_MAUG_BOX_FLOATS, MAXD = PARC_MAUG_MAX_DIM;
constexpr int WAVE_CELLS = 1024, WG_THREADS = 256;
constexpr int DIM_CAP = 1 << 20;           // what an out-of-range point count is stored as (the host refuses anything above MAXD)

struct Cfg {                               // by value
    int mode, pad, slice, B, nb0, nb1;
    float head0, head1, xs0, xs1, ys0, ys1;            // heading (degrees), x / y scale ranges
    float hs0, hs_a, hs_b0, hs_len;                    // height scale: [hs0, hs0 + hs_a) and [hs_b0, ..) of total length hs_len
    float len0, len1, ang0, ang1, bh0, bh1;            // boxes: side length (cells), angle, height ranges
    int jswap[PARC_MAX_BODIES], cswap[PARC_MAX_BODIES];   // left / right partner of every joint and contact column (itself when none)
};
struct Lib {                               // per clip, beside ClipArrays
    const float *maxmin;                   // [cells][2] or NULL
    const float *ring;                     // [C][2] what the pad ring reads for hf_maxmin: max of max, min of min
    const float *pgeom;                    // [C][4] the padded terrain's min point, dx, dy
    const int *win;                        // [C] int(round(fps * max_motion_len))
    const float *cdf;                      // [C] running sum of the normalised sample weights
};
struct PlanD { int *src, *start, *nframes; float *heading, *scale; int *mirror; float *hscale; int *nboxes, *box_frame; float *boxes; };
struct Run {                               // device arrays of one run (the handle owns them until the next run)
    int *cnt_f, *cnt_c;                    // [n] frames, cells
    long long *frame_off, *cell_off;       // [n + 1]
    float *vgeo;                           // [n][4] the slice's min grid point on the source terrain, and minus canon_xy
    int *src, *hf_dims; float *hf_geom, *canon_z;
    float *root_pos, *root_rot, *joint_rot, *contacts, *hf, *hf_maxmin;
};
struct Var { int c, start, nf, mirror, nb; float heading, sx, sy, hscale; };

// ---- the draws (shared by k_maug_draw and the DRAW = true kernels) ------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ctr_hi(unsigned long long v) { return (1ull << 62) | v; }
__device__ __forceinline__ float scale_u(float u, float lo, float hi) { return u * (hi - lo) + lo; }
__device__ __forceinline__ int randint_incl(float u, int m) { const int v = (int)(u * (float)(m + 1)); return v < m ? v : m; }

__device__ __forceinline__ Var draw_var(const Cfg &G, const ClipArrays &K, const Lib &L, unsigned long long seed, unsigned long long idx, int mirror) {
    float u[4], w[4];
    philox4(seed, ctr_hi(idx), 0u, u);
    philox4(seed, ctr_hi(idx), 1u, w);
    const int C = K.C;
    const float x = u[0] * L.cdf[C - 1];                       // torch.multinomial with replacement = inverse CDF per draw
    int lo = 0, hi = C - 1;
    while (lo < hi) { const int md = (lo + hi) >> 1; if (L.cdf[md] > x) hi = md; else lo = md + 1; }
    const int n = (int)(K.frame_off[lo + 1] - K.frame_off[lo]), mf = L.win[lo];
    Var V;
    V.c = lo;
    if (n > mf) { V.start = randint_incl(u[1], n - mf - 1); V.nf = mf; }   // random.randint(0, n - max_frames - 1) (:156)
    else { V.start = 0; V.nf = n; }
    V.heading = (scale_u(u[2], G.head0, G.head1) * 3.14159265358979323846f) / 180.0f;   // :161-162
    V.sx = scale_u(w[0], G.xs0, G.xs1); V.sy = scale_u(w[1], G.ys0, G.ys1);
    const float t = w[2] * G.hs_len;                           // uniform on [min, max] minus the open bad range = the reference's rejection loop
    V.hscale = t < G.hs_a ? G.hs0 + t : G.hs_b0 + (t - G.hs_a);
    V.nb = G.mode == PARC_MAUG_BOXES_ALONG_PATH ? G.nb0 + randint_incl(w[3], G.nb1 - G.nb0) : 0;
    V.mirror = mirror;
    return V;
}
// box b of variation idx: the frame it sits under, and len x, len y (cells), angle, height
__device__ __forceinline__ void draw_box(const Cfg &G, unsigned long long seed, unsigned long long idx, int b, int nf, int &frame, float *o) {
    float u[4], w[4];
    philox4(seed, ctr_hi(idx), 2u + 2u * b, u);
    philox4(seed, ctr_hi(idx), 3u + 2u * b, w);
    const int f = (int)(u[0] * (float)nf);                     // torch.randint(0, num_frames)
    frame = f < nf - 1 ? f : nf - 1;
    o[0] = scale_u(u[1], G.len0, G.len1); o[1] = scale_u(u[2], G.len0, G.len1);
    o[2] = scale_u(u[3], G.ang0, G.ang1);
    o[3] = scale_u(w[0], G.bh0, G.bh1);
}

// variation v of the launch: drawn, or read from the plan with every index clamped into its range (memory safety; the status word
// records that a clamp happened)
template <bool DRAW>
__device__ __forceinline__ Var get_var(const Cfg &G, const ClipArrays &K, const Lib &L, const PlanD &P, long long v, unsigned long long seed,
                                       unsigned long long first, int mirror, int *status) {
    if (DRAW) return draw_var(G, K, L, seed, first + (unsigned long long)v, mirror);
    Var V;
    bool bad = false;
    int c = P.src[v];
    if (c < 0 || c >= K.C) { bad = true; c = c < 0 ? 0 : K.C - 1; }
    const int n = (int)(K.frame_off[c + 1] - K.frame_off[c]);
    int s = P.start[v];
    if (s < 0 || s >= n) { bad = true; s = s < 0 ? 0 : n - 1; }
    int nf = P.nframes[v];
    if (nf < 1 || nf > n - s) { bad = true; nf = nf < 1 ? 1 : n - s; }
    int nb = G.mode == PARC_MAUG_BOXES_ALONG_PATH ? P.nboxes[v] : 0;
    if (nb < 0 || nb > MAXB) { bad = true; nb = nb < 0 ? 0 : MAXB; }
    V.c = c; V.start = s; V.nf = nf; V.nb = nb;
    V.mirror = P.mirror[v] != 0;
    V.heading = P.heading[v]; V.sx = P.scale[2 * v]; V.sy = P.scale[2 * v + 1];
    V.hscale = G.mode == PARC_MAUG_HEIGHT_SCALE ? P.hscale[v] : 1.f;
    if (bad) atomicOr(status, PARC_MAUG_STATUS_CLAMPED);
    return V;
}

// lane per variation (the boxes of a variation in its lane's loop: at most PARC_MAUG_MAX_BOXES)
__global__ void k_maug_draw(ClipArrays K, Lib L, Cfg G, PlanD P, long long n, unsigned long long seed, unsigned long long first, int mirror) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const Var V = draw_var(G, K, L, seed, first + (unsigned long long)v, mirror);
    P.src[v] = V.c; P.start[v] = V.start; P.nframes[v] = V.nf; P.heading[v] = V.heading; P.scale[2 * v] = V.sx; P.scale[2 * v + 1] = V.sy;
    P.mirror[v] = V.mirror; P.hscale[v] = V.hscale; P.nboxes[v] = V.nb;
    for (int b = 0; b < MAXB; ++b) {
        int fr = 0;
        float o[BF] = {0.f, 0.f, 0.f, 0.f};
        if (b < V.nb) draw_box(G, seed, first + (unsigned long long)v, b, V.nf, fr, o);
        P.box_frame[v * MAXB + b] = fr;
        for (int k = 0; k < BF; ++k) P.boxes[(v * MAXB + b) * BF + k] = o[k];
    }
}

template <bool DRAW>
__global__ void k_maug_layout(ClipArrays K, Lib L, Cfg G, PlanD P, int *cnt_f, long long n, unsigned long long seed, unsigned long long first, int *status) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    cnt_f[v] = get_var<DRAW>(G, K, L, P, v, seed, first, 0, status).nf;
}

// off[0 .. n] = exclusive scan of cnt[0 .. n): one block, a run of consecutive counts per thread, the block's partial sums through LDS
__global__ void __launch_bounds__(1024) k_maug_scan(const int *cnt, long long *off, long long n) {
    __shared__ long long s[1024];
    const int tid = threadIdx.x;
    const long long per = (n + 1023) / 1024, b = tid * per, e = b + per < n ? b + per : n;
    long long sum = 0;
    for (long long i = b; i < e; ++i) sum += cnt[i];
    s[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long t = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    long long run = s[tid] - sum;
    for (long long i = b; i < e; ++i) { off[i] = run; run += cnt[i]; }
    if (tid == 1023) off[n] = s[1023];
}

// ---- frames -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_min(float v) { for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64)); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64)); return v; }

// SubTerrain.round_point_to_grid_point (terrain_util.py:143)
__device__ __forceinline__ float round_to_grid(float p, float mn, float dx) { return rintf((p - mn) / dx) * dx + mn; }
// len(torch.arange(start, end, step)) on 0-dim fp32 tensors: ceil((end - start) / step) in double; 0 = not a count (NaN or < 1)
__device__ __forceinline__ int arange_count(float start, float end, float step) {
    const double c = ceil(((double)end - (double)start) / (double)step);
    return c >= 1.0 ? (c <= (double)DIM_CAP ? (int)c : DIM_CAP) : 0;
}
// point i of that arange: start + i * step, formed in double and stored as fp32
__device__ __forceinline__ float arange_point(float start, int i, float step) { return (float)((double)start + (double)i * (double)step); }

// the source cell under point (px, py) of the padded terrain of a clip (get_grid_index on the padded dims), -1 in the pad ring
__device__ __forceinline__ long long padded_cell(const float *pg, int pad, long long X0, long long Y0, float px, float py) {
    const long long i = grid_index(px, pg[0], pg[2], X0 + 2 * pad) - pad, j = grid_index(py, pg[1], pg[3], Y0 + 2 * pad) - pad;
    return (i >= 0 && i < X0 && j >= 0 && j < Y0) ? i * Y0 + j : -1;
}

// Joint.rot_to_dof then Joint.dof_to_rot (kin_char_model.py:61-105) of the flipped quaternion of joint p, rebuilt as joint j = its mirror
__device__ __forceinline__ Q4 mirror_joint(const CharTree &M, int p, int j, Q4 q) {
    q = mk4(q.x, -q.y, q.z, -q.w);                             // flip_quat_about_XZ_plane
    const int t = M.jtype[p];
    if (t == PARC_JOINT_HINGE) {
        V3 ax; float ang;
        quat_to_axis_angle(q, ax, ang);
        if (M.axis[p][0] * ax.x + M.axis[p][1] * ax.y + M.axis[p][2] * ax.z < 0.f) ang = ang * -1.f;
        return axis_angle_to_quat(mk3(M.axis[j][0], M.axis[j][1], M.axis[j][2]), ang);
    }
    if (t == PARC_JOINT_SPHERICAL) return exp_map_to_quat(quat_to_exp_map(q));
    return mk4(0.f, 0.f, 0.f, 1.f);
}

template <bool DRAW>
__global__ void __launch_bounds__(64) k_maug_frames(const CharTree *Mp, ClipArrays K, Lib L, Cfg G, PlanD P, Run R, unsigned long long seed,
                                                    unsigned long long first, int mirror, int *status) {
    const CharTree &M = *Mp;
    const long long v = blockIdx.x;
    const int lane = threadIdx.x, B = G.B, J = B - 1;
    const Var V = get_var<DRAW>(G, K, L, P, v, seed, first, mirror, status);
    const int c = V.c, nf = V.nf;
    const long long f0 = K.frame_off[c] + V.start, fo = R.frame_off[v];
    const float ch = cosf(V.heading), sh = sinf(V.heading);
    const Q4 hq = axis_angle_to_quat(mk3(0.f, 0.f, 1.f), V.heading);
    // 1. heading and scale; the turned frames wait in the output rows of their own lane
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY, x0 = 0.f, y0 = 0.f;
    bool nan = false;
    for (int f = lane; f < nf; f += 64) {
        const V3 p = ld3(K.src_root_pos + 3 * (f0 + f));
        const float x = (p.x * ch - p.y * sh) * V.sx, y = (p.x * sh + p.y * ch) * V.sy;     // rotate_2d_vec, then *= scale (:163-171)
        if (f == 0) { x0 = x; y0 = y; }
        nan |= (x != x) || (y != y);
        mnx = fminf(mnx, x); mny = fminf(mny, y); mxx = fmaxf(mxx, x); mxy = fmaxf(mxy, y);
        st3(R.root_pos + 3 * (fo + f), mk3(x, y, p.z));
        st4(R.root_rot + 4 * (fo + f), exp_map_to_quat(quat_to_exp_map(qmul(hq, ld4(K.src_root_rot + 4 * (f0 + f))))));
    }
    mnx = wave_min(mnx); mny = wave_min(mny); mxx = wave_max(mxx); mxy = wave_max(mxy);
    // torch.min / max propagate NaN; an infinite bound (an infinite scale) is no slice either: both end as the 1 x 1 slice below
    if (__any(nan) || !isfinite(mnx) || !isfinite(mny) || !isfinite(mxx) || !isfinite(mxy)) mnx = mny = mxx = mxy = NAN;
    // 2. the slice (wave-uniform): slice_terrain_around_motion :1592-1606, :1619-1640 on the padded terrain
    const float *pg = L.pgeom + 4 * c;
    const float dx = pg[2], dy = pg[3];
    const long long X0 = K.hf_dims[2 * c], Y0 = K.hf_dims[2 * c + 1];
    float mgx = pg[0], mgy = pg[1], cx = 0.f, cy = 0.f, cz = 0.f;
    int X = (int)X0 + 2 * G.pad, Y = (int)Y0 + 2 * G.pad;
    if (G.slice) {
        const float pad = dx * 2.f;                            // padding = terrain.dxdy[0].item() * 2 on both axes (:177)
        mgx = round_to_grid(mnx - pad, pg[0], dx); mgy = round_to_grid(mny - pad, pg[1], dy);
        X = arange_count(mgx, round_to_grid(mxx + pad, pg[0], dx) + dx, dx);
        Y = arange_count(mgy, round_to_grid(mxy + pad, pg[1], dy) + dy, dy);
        if (X < 1 || Y < 1) { if (lane == 0) atomicOr(status, PARC_MAUG_STATUS_NOT_FINITE); X = X < 1 ? 1 : X; Y = Y < 1 ? 1 : Y; }
        cx = __shfl(x0, 0, 64); cy = __shfl(y0, 0, 64);
    }
    const float lminx = mgx - cx, lminy = mgy - cy;            // min_x = min_grid_point - canon_xy
    if (G.slice) {                                             // get_hf_val_from_points(localised frame 0 = (0, 0)) on the sliced terrain (:1638)
        const int i0 = (int)grid_index(0.f, lminx, dx, X), j0 = (int)grid_index(0.f, lminy, dy, Y);
        const long long cell = padded_cell(pg, G.pad, X0, Y0, arange_point(mgx, i0, dx), arange_point(mgy, j0, dy));
        cz = cell >= 0 ? K.hf[K.hf_off[c] + cell] : 0.f;
    }
    // 3. localise (and mirror) the root; every lane rereads the rows it wrote
    for (int f = lane; f < nf; f += 64) {
        float *rp = R.root_pos + 3 * (fo + f);
        float x = rp[0] - cx, y = rp[1] - cy;
        const float z = rp[2] - cz;
        if (V.mirror) {                                        // flip_motion_about_XZ_plane :397-412
            y = y * -1.0f;
            const V3 e = quat_to_exp_map(ld4(R.root_rot + 4 * (fo + f)));
            st4(R.root_rot + 4 * (fo + f), exp_map_to_quat(mk3(e.x * -1.0f, (e.y * -1.0f) * -1.0f, e.z * -1.0f)));
        }
        st3(rp, mk3(x, y, z));
    }
    // 4. joints and contacts of the window, coalesced over (frame, joint) / (frame, body)
    for (int it = lane; it < nf * J; it += 64) {
        const int f = it / J, j = it - f * J + 1;
        Q4 q;
        if (V.mirror) { const int p = G.jswap[j]; q = mirror_joint(M, p, j, ld4(K.src_jrot + ((f0 + f) * J + p - 1) * 4)); }
        else q = *(const float4 *)(K.src_jrot + ((f0 + f) * J + j - 1) * 4);
        *(float4 *)(R.joint_rot + ((fo + f) * J + j - 1) * 4) = q;
    }
    for (int it = lane; it < nf * B; it += 64) {
        const int f = it / B, b = it - f * B;
        R.contacts[(fo + f) * B + b] = K.contacts[(f0 + f) * B + (V.mirror ? G.cswap[b] : b)];
    }
    if (lane == 0) {
        R.src[v] = c;
        R.hf_dims[2 * v] = X; R.hf_dims[2 * v + 1] = Y;
        R.cnt_c[v] = (!G.slice || (X <= MAXD && Y <= MAXD)) ? X * Y : 0;   // the limit is the slice's; an unsliced terrain keeps its size
        float *g = R.hf_geom + 4 * v;
        // flip_by_XZ_axis :189-190: min_point[1] = -1.0 * get_max_point()[1], get_max_point = min_point + dims * dxdy - dxdy
        g[0] = lminx; g[1] = V.mirror ? -1.0f * ((lminy + (float)Y * dy) - dy) : lminy; g[2] = dx; g[3] = dy;
        R.canon_z[v] = cz;
        float *vg = R.vgeo + 4 * v;
        vg[0] = mgx; vg[1] = mgy; vg[2] = lminx; vg[3] = lminy;
    }
}

// ---- terrain ------------------------------------------------------------------------------------------------------------------------
constexpr int BS = 9;                      // cx, cy, cos, sin, x0, x1, y0, y1, h (k_tgen_boxes' record: read wave-uniformly)
// add_boxes_to_hf_at_xy_points' test of cell (x, y) (:950-960): the construction of add_boxes_to_hf2, with the centre under a frame
__device__ __forceinline__ bool box_hit(const float *d, float x, float y) {
    const float ux = x - d[0], uy = y - d[1];
    const float rx = (ux * d[2] - uy * d[3]) + d[0], ry = (ux * d[3] + uy * d[2]) + d[1];   // rotate_2d_vec(xy - center) + center
    return rx < d[5] && rx > d[4] && ry < d[7] && ry > d[6];
}

template <bool DRAW>
__global__ void __launch_bounds__(WG_THREADS) k_maug_terrain(ClipArrays K, Lib L, Cfg G, PlanD P, Run R, unsigned long long seed, unsigned long long first,
                                                             int mirror, int *status) {
    __shared__ float s_b[MAXB * BS];
    const long long v = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int X = R.hf_dims[2 * v], Y = R.hf_dims[2 * v + 1], NP = R.cnt_c[v];   // 0: a refused slice
    const Var V = get_var<DRAW>(G, K, L, P, v, seed, first, mirror, status);
    const int c = V.c;
    const float *pg = L.pgeom + 4 * c, *vg = R.vgeo + 4 * v;
    const float dx = pg[2], dy = pg[3], mgx = vg[0], mgy = vg[1], cz = R.canon_z[v];
    const long long X0 = K.hf_dims[2 * c], Y0 = K.hf_dims[2 * c + 1], src0 = K.hf_off[c], cell0 = R.cell_off[v], fo = R.frame_off[v];
    if (G.mode == PARC_MAUG_BOXES_ALONG_PATH) {
        for (int b = tid; b < V.nb; b += nt) {
            int fr;
            float o[BF];
            if (DRAW) draw_box(G, seed, first + (unsigned long long)v, b, V.nf, fr, o);
            else {
                fr = P.box_frame[v * MAXB + b];
                for (int k = 0; k < BF; ++k) o[k] = P.boxes[(v * MAXB + b) * BF + k];
                if (fr < 0 || fr >= V.nf) { atomicOr(status, PARC_MAUG_STATUS_CLAMPED); fr = fr < 0 ? 0 : V.nf - 1; }
            }
            const float *rp = R.root_pos + 3 * (fo + fr);      // the localised frame; the mirror negated its y after the edit
            const float bx = (rp[0] - vg[2]) / dx, by = ((V.mirror ? -rp[1] : rp[1]) - vg[3]) / dy;   // (xy - min_point) / dxdy (:191-192)
            float *d = s_b + b * BS;
            d[0] = bx; d[1] = by; d[2] = cosf(o[2]); d[3] = sinf(o[2]);
            d[4] = bx - o[0] / 2.f; d[5] = bx + o[0] / 2.f; d[6] = by - o[1] / 2.f; d[7] = by + o[1] / 2.f;
            d[8] = o[3];
        }
        __syncthreads();
    }
    for (int p = tid; p < NP; p += nt) {
        const int i = p / Y, jo = p - i * Y, j = V.mirror ? Y - 1 - jo : jo;   // torch.flip(hf, dims=[1])
        long long cell;
        if (G.slice) cell = padded_cell(pg, G.pad, X0, Y0, arange_point(mgx, i, dx), arange_point(mgy, j, dy));
        else { const long long a = i - G.pad, b = j - G.pad; cell = (a >= 0 && a < X0 && b >= 0 && b < Y0) ? a * Y0 + b : -1; }
        float h = (cell >= 0 ? K.hf[src0 + cell] : 0.f) - cz;  // sliced_hf - canon_z (:1640)
        if (G.mode == PARC_MAUG_HEIGHT_SCALE) h = V.hscale * h;
        else if (G.mode == PARC_MAUG_BOXES_ALONG_PATH) {
            for (int b = V.nb - 1; b >= 0; --b)                // a later box overwrites: the last hit wins
                if (box_hit(s_b + b * BS, (float)i, (float)j)) { h = s_b[b * BS + 8]; break; }
        }
        R.hf[cell0 + p] = h;
        if (R.hf_maxmin) {
            R.hf_maxmin[2 * (cell0 + p)] = cell >= 0 ? L.maxmin[2 * (src0 + cell)] : L.ring[2 * c];
            R.hf_maxmin[2 * (cell0 + p) + 1] = cell >= 0 ? L.maxmin[2 * (src0 + cell) + 1] : L.ring[2 * c + 1];
        }
    }
}

// ---- validate -----------------------------------------------------------------------------------------------------------------------
enum { VB_SRC = 0, VB_START, VB_NFRAMES, VB_HEADING, VB_SCALE, VB_MIRROR, VB_HSCALE, VB_NBOXES, VB_BOX_FRAME, VB_BOXES, VB_COUNT };
__global__ void k_maug_validate(ClipArrays K, Cfg G, PlanD P, long long n, int *bits) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int bad = 0;
    const int c = P.src[v];
    if (c < 0 || c >= K.C) bad |= 1 << VB_SRC;
    else {
        const int nc = (int)(K.frame_off[c + 1] - K.frame_off[c]), s = P.start[v], nf = P.nframes[v];
        if (s < 0 || s >= nc) bad |= 1 << VB_START;
        else if (nf < 1 || nf > nc - s) bad |= 1 << VB_NFRAMES;
        else if (G.mode == PARC_MAUG_BOXES_ALONG_PATH) {
            const int nb = P.nboxes[v];
            if (nb < 0 || nb > MAXB) bad |= 1 << VB_NBOXES;
            else for (int b = 0; b < nb; ++b) {
                const int fr = P.box_frame[v * MAXB + b];
                if (fr < 0 || fr >= nf) bad |= 1 << VB_BOX_FRAME;
                for (int k = 0; k < BF; ++k) if (!isfinite(P.boxes[(v * MAXB + b) * BF + k])) bad |= 1 << VB_BOXES;
            }
        }
    }
    if (!isfinite(P.heading[v])) bad |= 1 << VB_HEADING;
    if (!isfinite(P.scale[2 * v]) || !isfinite(P.scale[2 * v + 1])) bad |= 1 << VB_SCALE;
    if (P.mirror[v] != 0 && P.mirror[v] != 1) bad |= 1 << VB_MIRROR;
    if (G.mode == PARC_MAUG_HEIGHT_SCALE && !isfinite(P.hscale[v])) bad |= 1 << VB_HSCALE;
    if (bad) atomicOr(bits, bad);
}

}  // namespace maug

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
struct ParcMotionAug : tool::CharHandle<parc::CharTree, DeviceEvents<8>> {   // mem: d_model, status
    struct Library {                      // what one parc_maug_set_clips loads
        DeviceArena mem;
        ClipArrays K{};
        maug::Lib L{};
    };
    struct Result {                       // what one run leaves: released by the next run, a new library, or with the handle
        DeviceArena mem;
        maug::Run R{};
        int n = 0;
        long long F = 0, cells = 0;
    };
    ParcMotionAugParams params{};
    maug::Cfg cfg{};
    std::unique_ptr<Library> lib;
    std::unique_ptr<Result> res;
    tool::StatusWords status;             // 0: the run kernels' word (parc_maug_plan_status), 1: the validate pass'
    bool drew = false;
};

extern "C" void parc_maug_destroy(ParcMotionAug *h) { tool::destroy(h); }

extern "C" int parc_maug_create(const ParcMotionAugParams *p, ParcMotionAug **out) {
    PARC_TRY(tool::create_args("maug", "ParcMotionAugParams", p, out, 2, false));
    if (p->mode < PARC_MAUG_HEIGHT_SCALE || p->mode > PARC_MAUG_NONE)
        return fail(PARC_ERR_INVALID, "maug: terrain_aug_type must be HEIGHT_SCALE, BOXES_ALONG_PATH or NONE");
    if (p->terrain_padding_size < 0 || p->terrain_padding_size > PARC_MAUG_MAX_DIM)
        return fail(PARC_ERR_INVALID, "maug: terrain_padding_size must be 0 .. PARC_MAUG_MAX_DIM = " + std::to_string(PARC_MAUG_MAX_DIM));
    const float ranges[][2] = {{p->min_heading_angle, p->max_heading_angle}, {p->x_scale[0], p->x_scale[1]}, {p->y_scale[0], p->y_scale[1]}};
    for (const auto &r : ranges) if (!std::isfinite(r[0]) || !std::isfinite(r[1])) return fail(PARC_ERR_INVALID, "maug: a heading or scale range is not finite");
    parc::CharTree M;
    PARC_TRY(tool::char_tree("maug", p->model, M));
    maug::Cfg G{};
    G.mode = p->mode; G.pad = p->terrain_padding_size; G.slice = p->slice_terrain != 0; G.B = M.B;
    G.head0 = p->min_heading_angle; G.head1 = p->max_heading_angle;
    G.xs0 = p->x_scale[0]; G.xs1 = p->x_scale[1]; G.ys0 = p->y_scale[0]; G.ys1 = p->y_scale[1];
    for (int b = 0; b < PARC_MAX_BODIES; ++b) { G.jswap[b] = b; G.cswap[b] = b; }
    for (int b = 0; b < M.B; ++b) {
        const int j = p->joint_swap[b], k = p->contact_swap[b];
        if (j < 0 || j >= M.B || k < 0 || k >= M.B || p->joint_swap[j] != b || p->contact_swap[k] != b || (b == 0 && j != 0))
            return fail(PARC_ERR_INVALID, "maug: joint_swap and contact_swap must pair bodies (swap[swap[b]] = b; the root with itself)");
        if (M.jtype[j] != M.jtype[b]) return fail(PARC_ERR_INVALID, "maug: joint " + std::to_string(b) + " and its mirror differ in type");
        G.jswap[b] = j; G.cswap[b] = k;
    }
    if (p->mode == PARC_MAUG_HEIGHT_SCALE) {
        const float lo = p->min_h_scale, hi = p->max_h_scale, b0 = p->bad_h_range[0], b1 = p->bad_h_range[1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi) || b0 != b0 || b1 != b1)
            return fail(PARC_ERR_INVALID, "maug: min_h_scale <= max_h_scale and bad_h_range must be numbers");
        G.hs0 = lo;
        if (b0 < b1 && b0 < hi && b1 > lo) {                   // the bad range cuts the range
            const float a_end = fmaxf(b0, lo), b_start = fminf(b1, hi);
            G.hs_a = a_end - lo; G.hs_b0 = b_start; G.hs_len = G.hs_a + (hi - b_start);
        } else { G.hs_a = hi - lo; G.hs_b0 = hi; G.hs_len = hi - lo; }
        if ((lo < hi && !(G.hs_len > 0.f)) || (lo == hi && b0 < lo && lo < b1))   // the reference's rejection loop would spin for ever
            return fail(PARC_ERR_INVALID, "maug: bad_h_range (" + std::to_string(b0) + ", " + std::to_string(b1) + ") swallows [min_h_scale, max_h_scale] = [" +
                                              std::to_string(lo) + ", " + std::to_string(hi) + "]: no height scale could be drawn");
    }
    if (p->mode == PARC_MAUG_BOXES_ALONG_PATH) {
        if (p->min_num_boxes < 0 || p->max_num_boxes < p->min_num_boxes || p->max_num_boxes > PARC_MAUG_MAX_BOXES)
            return fail(PARC_ERR_INVALID, "maug: 0 <= min_num_boxes <= max_num_boxes = " + std::to_string(p->max_num_boxes) + " <= PARC_MAUG_MAX_BOXES = " +
                                              std::to_string(PARC_MAUG_MAX_BOXES));
        const float r[] = {p->min_len, p->max_len, p->min_angle, p->max_angle, p->min_h, p->max_h};
        for (float x : r) if (!std::isfinite(x)) return fail(PARC_ERR_INVALID, "maug: a box range is not finite");
        G.nb0 = p->min_num_boxes; G.nb1 = p->max_num_boxes;
        G.len0 = p->min_len; G.len1 = p->max_len; G.ang0 = p->min_angle; G.ang1 = p->max_angle; G.bh0 = p->min_h; G.bh1 = p->max_h;
    }
    return tool::create("maug", p->device, M, out, [&](ParcMotionAug &h) -> int {
        h.params = *p; h.cfg = G;
        return h.status.alloc(h.mem, 2);
    });
}

// as parc_msamp_set_clips: validate; release the old library (and its results); build the new one in a local; install it last
extern "C" int parc_maug_set_clips(ParcMotionAug *h, const ParcMotionOptClips *c, const ParcMotionAugClipInfo *info) {
    if (!h || !c || !info) return fail(PARC_ERR_INVALID, "maug: null argument");
    PARC_TRY(clip_batch_arrays("maug", c));
    if (!info->fps_host || !info->max_frames_host) return fail(PARC_ERR_INVALID, "maug: null clip array");
    ClipBatch cb;
    PARC_TRY(clip_batch_clips("maug", c, cb));
    const int C = cb.C, pad = h->cfg.pad;
    std::vector<float> cdf((size_t)C), ring((size_t)2 * C), pgeom((size_t)4 * C), len((size_t)C);
    double wsum = 0.0;
    for (int i = 0; i < C; ++i) {
        const long long nf = c->frame_off_host[i + 1] - c->frame_off_host[i];
        if (info->fps_host[i] < 1) return fail(PARC_ERR_INVALID, "maug: fps must be >= 1");
        if (info->max_frames_host[i] < 1) return fail(PARC_ERR_INVALID, "maug: max_motion_len gives clip " + std::to_string(i) + " a window of no frames");
        if (nf > 0x7fffffffLL) return fail(PARC_ERR_INVALID, "maug: a clip has too many frames");
        len[(size_t)i] = h->params.sample_weight_by_length ? (float)((double)nf / (double)info->fps_host[i]) : 1.0f;   // frames / fps as fp32 (:92-94)
        wsum += len[(size_t)i];
        const float *g = c->hf_geom_host + 4 * i;
        pgeom[(size_t)4 * i] = g[0] - g[2] * (float)pad; pgeom[(size_t)4 * i + 1] = g[1] - g[3] * (float)pad;   // min_point -= dxdy * padding_size
        pgeom[(size_t)4 * i + 2] = g[2]; pgeom[(size_t)4 * i + 3] = g[3];
        float mx = -INFINITY, mn = INFINITY;                   // SubTerrain.pad :246-247
        if (info->hf_maxmin_host)
            for (long long k = c->hf_off_host[i]; k < c->hf_off_host[i + 1]; ++k) { mx = fmaxf(mx, info->hf_maxmin_host[2 * k]); mn = fminf(mn, info->hf_maxmin_host[2 * k + 1]); }
        ring[(size_t)2 * i] = mx; ring[(size_t)2 * i + 1] = mn;
    }
    float run = 0.f;
    for (int i = 0; i < C; ++i) { run += (float)(len[(size_t)i] / wsum); cdf[(size_t)i] = run; }
    HIPCHK(hipSetDevice(h->device));
    h->res.reset();
    std::unique_ptr<ParcMotionAug::Library> nl;
    PARC_TRY(tool::renew("maug", h->lib, nl));
    PARC_TRY(clip_batch_upload(nl->mem, nl->K, c, cb, h->host_model.B));
    maug::Lib &L = nl->L;
    if (info->hf_maxmin_host) PARC_TRY(nl->mem.alloc(L.maxmin, 2 * cb.ncell, info->hf_maxmin_host));
    PARC_TRY(nl->mem.alloc(L.ring, 2 * C, ring.data()));
    PARC_TRY(nl->mem.alloc(L.pgeom, 4 * C, pgeom.data()));
    PARC_TRY(nl->mem.alloc(L.win, C, info->max_frames_host));
    PARC_TRY(nl->mem.alloc(L.cdf, C, cdf.data()));
    h->lib = std::move(nl);
    return PARC_OK;
}

static maug::PlanD maug_plan(const ParcMotionAugPlan *p) {
    maug::PlanD d{};
    if (p) {
        d.src = (int *)p->src_clip; d.start = (int *)p->start_frame; d.nframes = (int *)p->num_frames; d.heading = (float *)p->heading;
        d.scale = (float *)p->scale; d.mirror = (int *)p->mirror; d.hscale = (float *)p->height_scale; d.nboxes = (int *)p->num_boxes;
        d.box_frame = (int *)p->box_frame; d.boxes = (float *)p->boxes;
    }
    return d;
}

static int maug_check_plan(ParcMotionAug *h, const ParcMotionAugPlan *p) {
    if (!h || !p) return fail(PARC_ERR_INVALID, "maug: null argument");
    if (!h->lib) return tool::no_clips("maug");
    if (p->n < 1) return fail(PARC_ERR_INVALID, "maug: n must be >= 1");
    if (!p->src_clip || !p->start_frame || !p->num_frames || !p->heading || !p->scale || !p->mirror || !p->height_scale || !p->num_boxes ||
        !p->box_frame || !p->boxes)
        return fail(PARC_ERR_INVALID, "maug: null plan array");
    return PARC_OK;
}

extern "C" int parc_maug_draw_plan(ParcMotionAug *h, uint64_t seed, uint64_t first_variation, int32_t mirror, const ParcMotionAugPlan *plan, void *stream) {
    PARC_TRY(maug_check_plan(h, plan));
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(h->ev[6], st));
    // the one call that writes through the plan's pointers: ParcMotionAugPlan declares them const for its readers, maug_plan casts that away
    PARC_TRY(tool::launch(maug::k_maug_draw, dim3(blocks(plan->n, 64)), dim3(64), 0, st, h->lib->K, h->lib->L, h->cfg, maug_plan(plan), (long long)plan->n,
                       (unsigned long long)seed, (unsigned long long)first_variation, mirror != 0));
    HIPCHK(hipEventRecord(h->ev[7], st));
    h->drew = true;
    return PARC_OK;
}

static int maug_validate(ParcMotionAug *h, const ParcMotionAugPlan *p, hipStream_t st) {
    static const char *names[maug::VB_COUNT] = {"src_clip: a clip index outside the library", "start_frame: outside its clip",
                                                "num_frames: a window that is empty or runs past its clip", "heading holds a value that is not finite",
                                                "scale holds a value that is not finite", "mirror must be 0 or 1",
                                                "height_scale holds a value that is not finite",
                                                "num_boxes: outside 0 .. PARC_MAUG_MAX_BOXES", "box_frame: outside its window",
                                                "boxes holds a value that is not finite"};
    PARC_TRY(h->status.clear(1, st));
    PARC_TRY(tool::launch(maug::k_maug_validate, dim3(blocks(p->n, 256)), dim3(256), 0, st, h->lib->K, h->cfg, maug_plan(p), (long long)p->n, h->status.d + 1));
    int v = 0;
    PARC_TRY(h->status.read(1, st, v));
    return v ? tool::bad_plan("maug", v, names) : PARC_OK;
}

template <bool DRAW>
static int maug_run(ParcMotionAug *h, int n, const ParcMotionAugPlan *plan, unsigned long long seed, unsigned long long first, int mirror, hipStream_t st,
                    ParcMotionAugSizes *sizes) {
    const maug::Cfg &G = h->cfg;
    const ClipArrays &K = h->lib->K;
    const maug::Lib &L = h->lib->L;
    const maug::PlanD P = maug_plan(plan);
    const int B = G.B, J = B - 1;
    std::unique_ptr<ParcMotionAug::Result> res;
    PARC_TRY(tool::renew("maug", h->res, res));
    maug::Run &R = res->R;
    DeviceArena &mem = res->mem;
    PARC_TRY(mem.alloc(R.cnt_f, n)); PARC_TRY(mem.alloc(R.cnt_c, n));
    PARC_TRY(mem.alloc(R.frame_off, n + 1LL)); PARC_TRY(mem.alloc(R.cell_off, n + 1LL));
    PARC_TRY(mem.alloc(R.vgeo, 4LL * n)); PARC_TRY(mem.alloc(R.src, n)); PARC_TRY(mem.alloc(R.hf_dims, 2LL * n));
    PARC_TRY(mem.alloc(R.hf_geom, 4LL * n)); PARC_TRY(mem.alloc(R.canon_z, n));
    // 1. frame counts -> offsets; the total comes back in one 8-byte copy
    HIPCHK(hipEventRecord(h->ev[0], st));
    PARC_TRY(tool::launch(maug::k_maug_layout<DRAW>, dim3(blocks(n, 256)), dim3(256), 0, st, K, L, G, P, R.cnt_f, (long long)n, seed, first, h->status.d));
    PARC_TRY(tool::launch(maug::k_maug_scan, dim3(1), dim3(1024), 0, st, R.cnt_f, R.frame_off, (long long)n));
    HIPCHK(hipEventRecord(h->ev[1], st));
    long long F = 0;
    HIPCHK(hipMemcpyAsync(&F, R.frame_off + n, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    PARC_TRY(mem.alloc(R.root_pos, 3 * F)); PARC_TRY(mem.alloc(R.root_rot, 4 * F));
    PARC_TRY(mem.alloc(R.joint_rot, 4 * F * J)); PARC_TRY(mem.alloc(R.contacts, F * B));
    // 2. frames and slices; the dims come back in one small copy
    HIPCHK(hipEventRecord(h->ev[2], st));
    PARC_TRY(tool::launch(maug::k_maug_frames<DRAW>, dim3((unsigned)n), dim3(64), 0, st, h->d_model, K, L, G, P, R, seed, first, mirror, h->status.d));
    PARC_TRY(tool::launch(maug::k_maug_scan, dim3(1), dim3(1024), 0, st, R.cnt_c, R.cell_off, (long long)n));
    HIPCHK(hipEventRecord(h->ev[3], st));
    std::vector<int> dims((size_t)2 * n);
    HIPCHK(hipMemcpyAsync(dims.data(), R.hf_dims, dims.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    long long cells = 0;
    int largest = 0;
    for (int v = 0; v < n; ++v) {
        const int X = dims[(size_t)2 * v], Y = dims[(size_t)2 * v + 1];
        if (G.slice && (X > PARC_MAUG_MAX_DIM || Y > PARC_MAUG_MAX_DIM))
            return fail(PARC_ERR_INVALID, "maug: the slice of variation " + std::to_string(v) + " is " + (X >= maug::DIM_CAP ? std::string("huge") : std::to_string(X)) +
                                              " x " + (Y >= maug::DIM_CAP ? std::string("huge") : std::to_string(Y)) + " cells; a side may have at most PARC_MAUG_MAX_DIM = " +
                                              std::to_string(PARC_MAUG_MAX_DIM));
        cells += (long long)X * Y;
        if (X * Y > largest) largest = X * Y;
    }
    PARC_TRY(mem.alloc(R.hf, cells));
    if (L.maxmin) PARC_TRY(mem.alloc(R.hf_maxmin, 2 * cells));
    // 3. terrain: one wave per variation while every slice of the launch has at most WAVE_CELLS cells, else one workgroup of 256
    HIPCHK(hipEventRecord(h->ev[4], st));
    PARC_TRY(tool::launch(maug::k_maug_terrain<DRAW>, dim3((unsigned)n), dim3(largest <= maug::WAVE_CELLS ? 64 : maug::WG_THREADS), 0, st, K, L, G, P, R, seed, first,
                       mirror, h->status.d));
    HIPCHK(hipEventRecord(h->ev[5], st));
    res->n = n; res->F = F; res->cells = cells;
    h->res = std::move(res);
    if (sizes) { sizes->n = n; sizes->total_frames = F; sizes->total_cells = cells; sizes->has_maxmin = L.maxmin != nullptr; }
    return PARC_OK;
}

extern "C" int parc_maug_augment_with(ParcMotionAug *h, const ParcMotionAugPlan *plan, int32_t validate, void *stream, ParcMotionAugSizes *sizes) {
    PARC_TRY(maug_check_plan(h, plan));
    HIPCHK(hipSetDevice(h->device));
    if (validate) PARC_TRY(maug_validate(h, plan, (hipStream_t)stream));
    return maug_run<false>(h, plan->n, plan, 0ull, 0ull, 0, (hipStream_t)stream, sizes);
}

extern "C" int parc_maug_augment(ParcMotionAug *h, int32_t n, uint64_t seed, uint64_t first_variation, int32_t mirror, void *stream, ParcMotionAugSizes *sizes) {
    if (!h) return fail(PARC_ERR_INVALID, "maug: null argument");
    if (!h->lib) return tool::no_clips("maug");
    if (n < 1) return fail(PARC_ERR_INVALID, "maug: n must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    return maug_run<true>(h, n, nullptr, (unsigned long long)seed, (unsigned long long)first_variation, mirror != 0, (hipStream_t)stream, sizes);
}

extern "C" int parc_maug_get_result(ParcMotionAug *h, const ParcMotionAugOutputs *o, void *stream) {
    if (!h || !o) return fail(PARC_ERR_INVALID, "maug: null argument");
    if (!h->res) return fail(PARC_ERR_STATE, "maug: nothing augmented yet");
    HIPCHK(hipSetDevice(h->device));
    const maug::Run &R = h->res->R;
    const long long n = h->res->n, F = h->res->F, cells = h->res->cells, B = h->cfg.B;
    if (o->hf_maxmin && !R.hf_maxmin) return fail(PARC_ERR_INVALID, "maug: the clips were loaded without hf_maxmin");
    struct Copy { void *dst; const void *src; size_t bytes; };
    const Copy copies[] = {{o->frame_off, R.frame_off, (size_t)(n + 1) * 8}, {o->cell_off, R.cell_off, (size_t)(n + 1) * 8}, {o->src_clip, R.src, (size_t)n * 4},
                           {o->hf_dims, R.hf_dims, (size_t)n * 8}, {o->hf_geom, R.hf_geom, (size_t)n * 16}, {o->canon_z, R.canon_z, (size_t)n * 4},
                           {o->root_pos, R.root_pos, (size_t)F * 12}, {o->root_rot, R.root_rot, (size_t)F * 16},
                           {o->joint_rot, R.joint_rot, (size_t)F * (B - 1) * 16}, {o->contacts, R.contacts, (size_t)F * B * 4},
                           {o->hf, R.hf, (size_t)cells * 4}, {o->hf_maxmin, R.hf_maxmin, (size_t)cells * 8}};
    for (const Copy &c : copies)
        if (c.dst && c.bytes) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PARC_OK;
}

extern "C" int parc_maug_plan_status(ParcMotionAug *h, void *stream, int32_t *status) {
    if (!h || !status) return fail(PARC_ERR_INVALID, "maug: null argument");
    HIPCHK(hipSetDevice(h->device));
    return h->status.take(0, (hipStream_t)stream, *status);
}

extern "C" int parc_maug_kernel_times(ParcMotionAug *h, float *ms4) {
    if (!h || !ms4) return fail(PARC_ERR_INVALID, "maug: null argument");
    const bool ran = h->res != nullptr;
    const tool::Span spans[] = {{h->drew, 6, 7}, {ran, 0, 1}, {ran, 2, 3}, {ran, 4, 5}};   // draw; layout, frames, terrain
    return tool::span_times("maug: nothing augmented yet", h->device, h->ev, spans, ms4);
}
