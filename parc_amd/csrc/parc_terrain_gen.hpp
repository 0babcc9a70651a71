// parc_terrain_gen.hpp — batched procedural terrain generator on gfx950 (parc_tgen_*, include/parc_env.h).
//
// Stage 2's BOXES / PATHS / STAIRS procgen modes (terrain_util.add_boxes_to_hf2 :861-917 without the hf_maxmin clamp, gen_paths_hf
// :541-592, add_stairs_to_hf :1002-1043 with draw_box :971-1000) for n terrains per call, one wave per terrain:
//   k_tgen_boxes   per-box constants (cos, sin, the four bounds) in LDS, lane per box; then every lane tests its cells against the boxes
//                  from the last to the first and keeps the first hit (= the reference's "a later box overwrites"); cells go straight
//                  to global, coalesced (a pure per-cell function needs no heightfield in LDS)
//   k_tgen_stairs  the same with per-stair constants; a cell walks the stairs and their steps backwards
//   k_tgen_paths   lane per path: the serial walk of PARC_TGEN_PATH_POINTS points (fp32, the reference's association), each point's cell
//                  gets atomicMax(path index) in an LDS plane (order-free: the highest index is the path painted last); then the heights
//                  are looked up and MaxPool2d(2 m + 1, 1, m) runs out of LDS as an x pass and a y pass (max is exact)
// Every kernel is a template on DRAW: false reads the plan's arrays, true draws the same values in place with the functions
// k_tgen_draw uses, so parc_tgen_generate gives the bits of parc_tgen_draw_plan + parc_tgen_generate_with.  Integer LDS atomics only.
// LDS: boxes 2.3 KB, stairs 0.8 KB (static); paths 8 B per cell (dynamic): 2 KB at 16 x 16, 32 KB at 64 x 64 (5 waves per CU there).
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
#include "parc_tool_handle.hpp"

namespace tgen {
using namespace parc;

constexpr int PTS = PARC_TGEN_PATH_POINTS;
constexpr int BF = PARC_TGEN_BOX_FLOATS, SF = PARC_TGEN_STAIR_FLOATS;
constexpr float TWO_PI = 6.283185307179586f;
static_assert(PTS % 4 == 0, "the walk consumes the turn normals four at a time");
static_assert(PARC_TGEN_MAX_PATHS <= 64 && (2 + PTS / 4) <= 256, "a lane per path; a path's counters fit its block of 256");

struct Cfg {                               // by value
    int mode, X, Y, nb, np, pool, ns;
    float dx, dy, minx, miny;
    float bh0, bh1, len0, len1, ang0, ang1;    // boxes: height, length, angle ranges
    float ph0, ph1, floor_h;                   // paths
    float sh0, sh1, st0, st1, th0, th1;        // stairs: start height, step height, thickness ranges
};
struct PlanD { float *boxes, *pstart, *pvy, *pangle, *pturn, *pheight, *stairs; };

// ---- the draws (shared by k_tgen_draw and the DRAW = true kernels) ---------------------------------------------------------------
__device__ __forceinline__ unsigned long long ctr_hi(int mode, unsigned long long t) { return (1ull << 61) | ((unsigned long long)mode << 56) | t; }
__device__ __forceinline__ float scale_u(float u, float lo, float hi) { return u * (hi - lo) + lo; }
// two normals from two uniforms: Box-Muller on (0, 1] (k_msamp_draw's form)
__device__ __forceinline__ void box_muller(float u0, float u1, float &z0, float &z1) {
    const float r = sqrtf(-2.f * logf(1.f - u0)), a = TWO_PI * u1;
    z0 = r * cosf(a); z1 = r * sinf(a);
}

__device__ __forceinline__ void draw_box(const Cfg &G, unsigned long long seed, unsigned long long t, int b, float *o) {
    float u[4], v[4];
    philox4(seed, ctr_hi(PARC_TGEN_BOXES, t), 2u * b, u);
    philox4(seed, ctr_hi(PARC_TGEN_BOXES, t), 2u * b + 1u, v);
    o[0] = u[0] * (float)G.X; o[1] = u[1] * (float)G.Y;                                     // rand(2) * hf.shape
    o[2] = scale_u(u[2], G.len0, G.len1); o[3] = scale_u(u[3], G.len0, G.len1);
    o[4] = scale_u(v[0], G.ang0, G.ang1);
    o[5] = scale_u(v[1], G.bh0, G.bh1);
}

struct PathHead { float sx, sy, vy, angle, height; };
__device__ __forceinline__ PathHead draw_path_head(const Cfg &G, unsigned long long seed, unsigned long long t, int p) {
    float u[4], v[4];
    philox4(seed, ctr_hi(PARC_TGEN_PATHS, t), 256u * p, u);
    philox4(seed, ctr_hi(PARC_TGEN_PATHS, t), 256u * p + 1u, v);
    PathHead h;
    // start = rand * (max_point - min_point) + min_point with max_point = dims * dxdy + min_point (:568-573), not get_max_point()
    h.sx = u[0] * (((float)G.X * G.dx + G.minx) - G.minx) + G.minx;
    h.sy = u[1] * (((float)G.Y * G.dy + G.miny) - G.miny) + G.miny;
    h.angle = (u[2] * 2.0f) * 3.14159265358979323846f;
    h.height = scale_u(u[3], G.ph0, G.ph1);
    float z1;
    box_muller(v[0], v[1], h.vy, z1);                                                       // the reference's randn(2) minus the discarded first
    return h;
}
__device__ __forceinline__ void draw_turn4(unsigned long long seed, unsigned long long t, int p, int k, float *z) {
    float u[4];
    philox4(seed, ctr_hi(PARC_TGEN_PATHS, t), 256u * p + 2u + (unsigned)k, u);
    box_muller(u[0], u[1], z[0], z[1]);
    box_muller(u[2], u[3], z[2], z[3]);
}

__device__ __forceinline__ void draw_stair(const Cfg &G, unsigned long long seed, unsigned long long t, int s, float *o) {
    float u[4], v[4];
    philox4(seed, ctr_hi(PARC_TGEN_STAIRS, t), 2u * s, u);
    philox4(seed, ctr_hi(PARC_TGEN_STAIRS, t), 2u * s + 1u, v);
    // rand * (get_max_point() - min_point) + min_point, get_max_point() = min_point + dims * dxdy - dxdy (terrain_util.py:136)
    const float rx = ((G.minx + (float)G.X * G.dx) - G.dx) - G.minx, ry = ((G.miny + (float)G.Y * G.dy) - G.dy) - G.miny;
    o[0] = u[0] * rx + G.minx; o[1] = u[1] * ry + G.miny;
    o[2] = u[2] * rx + G.minx; o[3] = u[3] * ry + G.miny;
    o[4] = scale_u(v[0], G.sh0, G.sh1);
    o[5] = scale_u(v[1], G.st0, G.st1);
    o[6] = scale_u(v[2], G.th0, G.th1);
}

// lane per box / path / stair (turn normals: lane per four)
__global__ void k_tgen_draw(Cfg G, PlanD P, long long n, unsigned long long seed, unsigned long long first) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (G.mode == PARC_TGEN_BOXES) {
        if (i >= n * G.nb) return;
        const long long t = i / G.nb;
        draw_box(G, seed, first + (unsigned long long)t, (int)(i - t * G.nb), P.boxes + i * BF);
    } else if (G.mode == PARC_TGEN_STAIRS) {
        if (i >= n * G.ns) return;
        const long long t = i / G.ns;
        draw_stair(G, seed, first + (unsigned long long)t, (int)(i - t * G.ns), P.stairs + i * SF);
    } else {
        constexpr int NQ = PTS / 4;
        if (i >= n * G.np * NQ) return;
        const long long tp = i / NQ, t = tp / G.np;
        const int k = (int)(i - tp * NQ), p = (int)(tp - t * G.np);
        float z[4];
        draw_turn4(seed, first + (unsigned long long)t, p, k, z);
        *(float4 *)(P.pturn + tp * PTS + 4 * k) = make_float4(z[0], z[1], z[2], z[3]);
        if (k == 0) {
            const PathHead h = draw_path_head(G, seed, first + (unsigned long long)t, p);
            P.pstart[2 * tp] = h.sx; P.pstart[2 * tp + 1] = h.sy; P.pvy[tp] = h.vy; P.pangle[tp] = h.angle; P.pheight[tp] = h.height;
        }
    }
}

// ---- BOXES --------------------------------------------------------------------------------------------------------------------------
constexpr int BS = 9;                      // cx, cy, cos, sin, x0, x1, y0, y1, h (read wave-uniformly: broadcasts)
template <bool DRAW>
__global__ void __launch_bounds__(64) k_tgen_boxes(Cfg G, PlanD P, float *hf, unsigned long long seed, unsigned long long first) {
    __shared__ float s_b[PARC_TGEN_MAX_BOXES * BS];
    const long long t = blockIdx.x;
    const int lane = threadIdx.x, NP = G.X * G.Y, nb = G.nb;
    for (int b = lane; b < nb; b += 64) {
        float o[BF];
        if (DRAW) draw_box(G, seed, first + (unsigned long long)t, b, o);
        else for (int k = 0; k < BF; ++k) o[k] = P.boxes[(t * nb + b) * BF + k];
        float *d = s_b + b * BS;
        d[0] = o[0]; d[1] = o[1]; d[2] = cosf(o[4]); d[3] = sinf(o[4]);
        d[4] = o[0] - o[2] / 2.f; d[5] = o[0] + o[2] / 2.f; d[6] = o[1] - o[3] / 2.f; d[7] = o[1] + o[3] / 2.f;
        d[8] = o[5];
    }
    __syncthreads();
    for (int p = lane; p < NP; p += 64) {
        const int ix = p / G.Y, iy = p - ix * G.Y;
        float h = 0.f;                                                       // SubTerrain starts at zeros
        for (int b = nb - 1; b >= 0; --b) {
            const float *d = s_b + b * BS;
            const float ux = (float)ix - d[0], uy = (float)iy - d[1];
            const float rx = (ux * d[2] - uy * d[3]) + d[0], ry = (ux * d[3] + uy * d[2]) + d[1];   // rotate_2d_vec(xy - center) + center
            if (rx < d[5] && rx > d[4] && ry < d[7] && ry > d[6]) { h = d[8]; break; }
        }
        hf[t * NP + p] = h;
    }
}

// ---- STAIRS -------------------------------------------------------------------------------------------------------------------------
constexpr int SS = 11;                     // start x, y, step dx, dy, cos, sin, steps, h0, step h, half width, half length
__device__ __forceinline__ int stair_steps(float sx, float sy, float ex, float ey, float dx) {
    const float ddx = ex - sx, ddy = ey - sy;
    const double nd = ceil((double)sqrtf(ddx * ddx + ddy * ddy) / (double)dx);       // int(np.ceil(norm.item() / dxdy[0].item()))
    return nd >= 0.0 ? (nd <= (double)PARC_TGEN_MAX_STEPS ? (int)nd : PARC_TGEN_MAX_STEPS + 1) : -1;   // -1: not a number
}

template <bool DRAW>
__global__ void __launch_bounds__(64) k_tgen_stairs(Cfg G, PlanD P, float *hf, unsigned long long seed, unsigned long long first) {
    __shared__ float s_s[PARC_TGEN_MAX_STAIRS * SS];
    __shared__ int s_n[PARC_TGEN_MAX_STAIRS];
    const long long t = blockIdx.x;
    const int lane = threadIdx.x, NP = G.X * G.Y, ns = G.ns;
    for (int s = lane; s < ns; s += 64) {
        float o[SF];
        if (DRAW) draw_stair(G, seed, first + (unsigned long long)t, s, o);
        else for (int k = 0; k < SF; ++k) o[k] = P.stairs[(t * ns + s) * SF + k];
        const float ddx = o[2] - o[0], ddy = o[3] - o[1];
        const int steps = stair_steps(o[0], o[1], o[2], o[3], G.dx);
        const float ang = -atan2f(ddy, ddx), fn = (float)steps;
        float *d = s_s + s * SS;
        d[0] = o[0]; d[1] = o[1]; d[2] = ddx / fn; d[3] = ddy / fn; d[4] = cosf(ang); d[5] = sinf(ang);
        d[7] = o[4]; d[8] = o[5]; d[9] = G.dx / 2.f; d[10] = o[6] / 2.f;
        s_n[s] = steps < 0 ? 0 : (steps > PARC_TGEN_MAX_STEPS ? PARC_TGEN_MAX_STEPS : steps);
    }
    __syncthreads();
    for (int p = lane; p < NP; p += 64) {
        const int ix = p / G.Y, iy = p - ix * G.Y;
        const float x = (float)ix * G.dx + G.minx, y = (float)iy * G.dy + G.miny;       // draw_box's cell centres :980-981
        float h = 0.f;
        bool hit = false;
        for (int s = ns - 1; s >= 0 && !hit; --s) {
            const float *d = s_s + s * SS;
            for (int j = s_n[s] - 1; j >= 0; --j) {
                const float cx = d[0] + (float)j * d[2], cy = d[1] + (float)j * d[3];   // stair_start + j * stair_dxdy
                const float ux = x - cx, uy = y - cy;
                const float rx = (ux * d[4] - uy * d[5]) + cx, ry = (ux * d[5] + uy * d[4]) + cy;
                if (rx < cx + d[9] && rx > cx - d[9] && ry < cy + d[10] && ry > cy - d[10]) {
                    h = (float)((double)d[7] + (double)j * (double)d[8]);                // start_height + j * step_height, in double
                    hit = true;
                    break;
                }
            }
        }
        hf[t * NP + p] = h;
    }
}

// ---- PATHS --------------------------------------------------------------------------------------------------------------------------
// round((x - min) / dx) half to even, clamped to [0, dim - 1]; not-a-number goes to 0 (the reference's int64 cast of NaN clamps there too)
__device__ __forceinline__ int path_index(float x, float mn, float dx, int dim) {
    const float r = rintf((x - mn) / dx);
    return r >= (float)(dim - 1) ? dim - 1 : (r > 0.f ? (int)r : 0);
}

template <bool DRAW>
__global__ void __launch_bounds__(64) k_tgen_paths(Cfg G, PlanD P, float *hf, unsigned long long seed, unsigned long long first) {
    extern __shared__ int s_mem[];                          // [cells] the painting path's index, later the x-pooled plane; [cells] heights
    __shared__ float s_h[PARC_TGEN_MAX_PATHS];
    const long long t = blockIdx.x;
    const int lane = threadIdx.x, X = G.X, Y = G.Y, NP = X * Y, np = G.np;
    int *s_idx = s_mem;
    float *s_tmp = (float *)s_mem, *s_hf = (float *)(s_mem + NP);
    for (int p = lane; p < NP; p += 64) s_idx[p] = -1;
    __syncthreads();
    if (lane < np) {
        const long long tp = t * np + lane;
        PathHead H;
        if (DRAW) H = draw_path_head(G, seed, first + (unsigned long long)t, lane);
        else { H.sx = P.pstart[2 * tp]; H.sy = P.pstart[2 * tp + 1]; H.vy = P.pvy[tp]; H.angle = P.pangle[tp]; H.height = P.pheight[tp]; }
        s_h[lane] = H.height;
        const float dt = (float)(1.0 / 30.0);
        const float c0 = cosf(H.angle), s0 = sinf(H.angle);
        float vx = 1.0f * c0 - H.vy * s0, vy = 1.0f * s0 + H.vy * c0;       // v = (1, vy) rotated by angle (:548-551)
        float px = H.sx, py = H.sy;
        for (int k = 0; k < PTS / 4; ++k) {
            float z[4];
            if (DRAW) draw_turn4(seed, first + (unsigned long long)t, lane, k, z);
            else { const float4 q = *(const float4 *)(P.pturn + tp * PTS + 4 * k); z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w; }
            for (int e = 0; e < 4; ++e) {
                atomicMax(&s_idx[path_index(px, G.minx, G.dx, X) * Y + path_index(py, G.miny, G.dy, Y)], lane);   // xy[i] = pos
                px = px + vx * dt; py = py + vy * dt;                                                             // pos += v * dt
                const float a = (z[e] * dt) * 7.0f, ca = cosf(a), sa = sinf(a);                                   // angle * dt * curviness
                const float nx = vx * ca - vy * sa, ny = vx * sa + vy * ca;
                vx = nx; vy = ny;
            }
        }
    }
    __syncthreads();
    for (int p = lane; p < NP; p += 64) { const int i = s_idx[p]; s_hf[p] = i < 0 ? G.floor_h : s_h[i]; }
    __syncthreads();
    const int m = G.pool;
    for (int p = lane; p < NP; p += 64) {                   // x pass; consecutive lanes read consecutive words in both passes
        const int ix = p / Y;
        const int a = ix - m > 0 ? ix - m : 0, b = ix + m < X - 1 ? ix + m : X - 1;
        float v = s_hf[p];
        for (int i = a; i <= b; ++i) v = fmaxf(v, s_hf[p + (i - ix) * Y]);
        s_tmp[p] = v;
    }
    __syncthreads();
    for (int p = lane; p < NP; p += 64) {
        const int ix = p / Y, iy = p - ix * Y;
        const int a = iy - m > 0 ? iy - m : 0, b = iy + m < Y - 1 ? iy + m : Y - 1;
        float v = s_tmp[p];
        for (int j = a; j <= b; ++j) v = fmaxf(v, s_tmp[p + (j - iy)]);
        hf[t * NP + p] = v;
    }
}

// ---- validate -----------------------------------------------------------------------------------------------------------------------
__global__ void k_tgen_validate(const float *a, long long count, int bit, int *status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && !isfinite(a[i])) atomicOr(status, bit);
}
__global__ void k_tgen_validate_steps(const float *stairs, long long count, float dx, int bit, int *status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float *o = stairs + i * SF;
    const int steps = stair_steps(o[0], o[1], o[2], o[3], dx);
    if (steps < 0 || steps > PARC_TGEN_MAX_STEPS) atomicOr(status, bit);
}

}  // namespace tgen

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
struct ParcTerrainGen : tool::Handle<DeviceEvents<4>> {   // mem: status
    tgen::Cfg cfg{};
    tool::StatusWords status;             // one word: the validate pass'
    bool drew = false, ran = false;
};

extern "C" void parc_tgen_destroy(ParcTerrainGen *h) { tool::destroy(h); }

extern "C" int parc_tgen_create(const ParcTerrainGenParams *p, ParcTerrainGen **out) {
    PARC_TRY(tool::create_args("tgen", "ParcTerrainGenParams", p, out));
    if (p->mode < PARC_TGEN_BOXES || p->mode > PARC_TGEN_STAIRS) return fail(PARC_ERR_INVALID, "tgen: mode must be PARC_TGEN_BOXES, PATHS or STAIRS");
    if (p->dim_x < 4 || p->dim_y < 4 || p->dim_x > PARC_TGEN_MAX_DIM || p->dim_y > PARC_TGEN_MAX_DIM)
        return fail(PARC_ERR_INVALID, "tgen: a " + std::to_string(p->dim_x) + " x " + std::to_string(p->dim_y) + " grid; sides must be 4 .. PARC_TGEN_MAX_DIM = " +
                                          std::to_string(PARC_TGEN_MAX_DIM) + " cells");
    if (!(p->dx > 0.f) || !(p->dy > 0.f)) return fail(PARC_ERR_INVALID, "tgen: dx and dy must be > 0");
    if (p->mode == PARC_TGEN_BOXES && (p->num_boxes < 1 || p->num_boxes > PARC_TGEN_MAX_BOXES))
        return fail(PARC_ERR_INVALID, "tgen: num_boxes = " + std::to_string(p->num_boxes) + " must be 1 .. PARC_TGEN_MAX_BOXES = " + std::to_string(PARC_TGEN_MAX_BOXES));
    if (p->mode == PARC_TGEN_PATHS && (p->num_terrain_paths < 1 || p->num_terrain_paths > PARC_TGEN_MAX_PATHS))
        return fail(PARC_ERR_INVALID, "tgen: num_terrain_paths = " + std::to_string(p->num_terrain_paths) + " must be 1 .. PARC_TGEN_MAX_PATHS = " +
                                          std::to_string(PARC_TGEN_MAX_PATHS));
    if (p->mode == PARC_TGEN_PATHS && (p->maxpool_size < 0 || p->maxpool_size > PARC_TGEN_MAX_POOL))
        return fail(PARC_ERR_INVALID, "tgen: maxpool_size = " + std::to_string(p->maxpool_size) + " must be 0 .. PARC_TGEN_MAX_POOL = " + std::to_string(PARC_TGEN_MAX_POOL));
    if (p->mode == PARC_TGEN_STAIRS && (p->num_stairs < 1 || p->num_stairs > PARC_TGEN_MAX_STAIRS))
        return fail(PARC_ERR_INVALID, "tgen: num_stairs = " + std::to_string(p->num_stairs) + " must be 1 .. PARC_TGEN_MAX_STAIRS = " + std::to_string(PARC_TGEN_MAX_STAIRS));
    return tool::create("tgen", p->device, out, [&](ParcTerrainGen &h) -> int {
        tgen::Cfg &G = h.cfg;
        G.mode = p->mode; G.X = p->dim_x; G.Y = p->dim_y; G.nb = p->num_boxes; G.np = p->num_terrain_paths; G.pool = p->maxpool_size; G.ns = p->num_stairs;
        G.dx = p->dx; G.dy = p->dy; G.minx = p->min_point[0]; G.miny = p->min_point[1];
        G.bh0 = p->min_box_h; G.bh1 = p->max_box_h; G.len0 = p->box_min_len; G.len1 = p->box_max_len; G.ang0 = p->min_box_angle; G.ang1 = p->max_box_angle;
        G.ph0 = p->path_min_height; G.ph1 = p->path_max_height; G.floor_h = p->floor_height;
        G.sh0 = p->min_stair_start_height; G.sh1 = p->max_stair_start_height; G.st0 = p->min_step_height; G.st1 = p->max_step_height;
        G.th0 = p->min_stair_thickness; G.th1 = p->max_stair_thickness;
        PARC_TRY(h.status.alloc(h.mem, 1));
        return h.ev.create();
    });
}

static tgen::PlanD tgen_plan(const ParcTerrainGenPlan *p) {
    tgen::PlanD d{};
    if (p) {
        d.boxes = (float *)p->boxes; d.pstart = (float *)p->path_start; d.pvy = (float *)p->path_vy; d.pangle = (float *)p->path_angle;
        d.pturn = (float *)p->path_turn; d.pheight = (float *)p->path_height; d.stairs = (float *)p->stairs;
    }
    return d;
}

static int tgen_check_plan(ParcTerrainGen *h, const ParcTerrainGenPlan *p) {
    if (!h || !p) return fail(PARC_ERR_INVALID, "tgen: null argument");
    if (p->n < 1) return fail(PARC_ERR_INVALID, "tgen: n must be >= 1");
    const int mode = h->cfg.mode;
    if (mode == PARC_TGEN_BOXES && !p->boxes) return fail(PARC_ERR_INVALID, "tgen: BOXES needs the plan's boxes");
    if (mode == PARC_TGEN_STAIRS && !p->stairs) return fail(PARC_ERR_INVALID, "tgen: STAIRS needs the plan's stairs");
    if (mode == PARC_TGEN_PATHS && (!p->path_start || !p->path_vy || !p->path_angle || !p->path_turn || !p->path_height))
        return fail(PARC_ERR_INVALID, "tgen: PATHS needs path_start, path_vy, path_angle, path_turn and path_height");
    if (mode == PARC_TGEN_PATHS && ((uintptr_t)p->path_turn & 15)) return fail(PARC_ERR_INVALID, "tgen: path_turn must be 16-byte aligned");
    return PARC_OK;
}

template <bool DRAW>
static int tgen_launch(ParcTerrainGen *h, int n, const tgen::PlanD &P, float *hf, unsigned long long seed, unsigned long long first, hipStream_t st) {
    const tgen::Cfg &G = h->cfg;
    HIPCHK(hipEventRecord(h->ev[2], st));
    if (G.mode == PARC_TGEN_BOXES)
        PARC_TRY(tool::launch(tgen::k_tgen_boxes<DRAW>, dim3((unsigned)n), dim3(64), 0, st, G, P, hf, seed, first));
    else if (G.mode == PARC_TGEN_STAIRS)
        PARC_TRY(tool::launch(tgen::k_tgen_stairs<DRAW>, dim3((unsigned)n), dim3(64), 0, st, G, P, hf, seed, first));
    else
        PARC_TRY(tool::launch(tgen::k_tgen_paths<DRAW>, dim3((unsigned)n), dim3(64), (size_t)G.X * G.Y * 2 * sizeof(float), st, G, P, hf, seed, first));
    HIPCHK(hipEventRecord(h->ev[3], st));
    h->ran = true;
    return PARC_OK;
}

extern "C" int parc_tgen_draw_plan(ParcTerrainGen *h, uint64_t seed, uint64_t first_terrain, const ParcTerrainGenPlan *plan, void *stream) {
    PARC_TRY(tgen_check_plan(h, plan));
    HIPCHK(hipSetDevice(h->device));
    const tgen::Cfg &G = h->cfg;
    const long long n = plan->n;
    const long long items = G.mode == PARC_TGEN_BOXES ? n * G.nb : (G.mode == PARC_TGEN_STAIRS ? n * G.ns : n * G.np * (tgen::PTS / 4));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(h->ev[0], st));
    PARC_TRY(tool::launch(tgen::k_tgen_draw, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, G, tgen_plan(plan), n, (unsigned long long)seed,
                       (unsigned long long)first_terrain));
    HIPCHK(hipEventRecord(h->ev[1], st));
    h->drew = true;
    return PARC_OK;
}

// the validate pass of parc_tgen_generate_with: synchronises; a bad field is PARC_ERR_INVALID by name
static int tgen_validate(ParcTerrainGen *h, const ParcTerrainGenPlan *p, hipStream_t st) {
    const tgen::Cfg &G = h->cfg;
    const long long n = p->n;
    struct Field { const char *name; const float *a; long long count; };
    constexpr int STEPS_BIT = 8;           // above the fields' bits (a mode has at most five)
    std::vector<Field> f;
    if (G.mode == PARC_TGEN_BOXES) f.push_back({"boxes", p->boxes, n * G.nb * tgen::BF});
    else if (G.mode == PARC_TGEN_STAIRS) f.push_back({"stairs", p->stairs, n * G.ns * tgen::SF});
    else {
        f.push_back({"path_start", p->path_start, n * G.np * 2}); f.push_back({"path_vy", p->path_vy, n * G.np});
        f.push_back({"path_angle", p->path_angle, n * G.np}); f.push_back({"path_turn", p->path_turn, n * G.np * tgen::PTS});
        f.push_back({"path_height", p->path_height, n * G.np});
    }
    PARC_TRY(h->status.clear(0, st));
    for (size_t k = 0; k < f.size(); ++k) {
        PARC_TRY(tool::launch(tgen::k_tgen_validate, dim3((unsigned)((f[k].count + 255) / 256)), dim3(256), 0, st, f[k].a, f[k].count, 1 << k, h->status.d));
    }
    if (G.mode == PARC_TGEN_STAIRS) {
        PARC_TRY(tool::launch(tgen::k_tgen_validate_steps, dim3((unsigned)((n * G.ns + 255) / 256)), dim3(256), 0, st, p->stairs, n * G.ns, G.dx, 1 << STEPS_BIT, h->status.d));
    }
    int v = 0;
    PARC_TRY(h->status.read(0, st, v));
    if (!v) return PARC_OK;
    std::string names[STEPS_BIT + 1];      // bit k: field k; the last: the stairs' step count
    for (size_t k = 0; k < f.size(); ++k) names[k] = std::string(f[k].name) + " holds a value that is not finite";
    names[STEPS_BIT] = "stairs: a stair needs more than PARC_TGEN_MAX_STEPS = " + std::to_string(PARC_TGEN_MAX_STEPS) + " steps";
    return tool::bad_plan("tgen", v, names);
}

extern "C" int parc_tgen_generate_with(ParcTerrainGen *h, const ParcTerrainGenPlan *plan, float *hf, int32_t validate, void *stream) {
    PARC_TRY(tgen_check_plan(h, plan));
    if (!hf) return fail(PARC_ERR_INVALID, "tgen: null output");
    HIPCHK(hipSetDevice(h->device));
    if (validate) PARC_TRY(tgen_validate(h, plan, (hipStream_t)stream));
    return tgen_launch<false>(h, plan->n, tgen_plan(plan), hf, 0ull, 0ull, (hipStream_t)stream);
}

extern "C" int parc_tgen_generate(ParcTerrainGen *h, int32_t n, uint64_t seed, uint64_t first_terrain, float *hf, void *stream) {
    if (!h || !hf) return fail(PARC_ERR_INVALID, "tgen: null argument");
    if (n < 1) return fail(PARC_ERR_INVALID, "tgen: n must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    return tgen_launch<true>(h, n, tgen_plan(nullptr), hf, (unsigned long long)seed, (unsigned long long)first_terrain, (hipStream_t)stream);
}

extern "C" int parc_tgen_kernel_times(ParcTerrainGen *h, float *ms2) {
    if (!h || !ms2) return fail(PARC_ERR_INVALID, "tgen: null argument");
    const tool::Span spans[] = {{h->drew, 0, 1}, {h->ran, 2, 3}};   // draw, generate
    return tool::span_times("tgen: nothing generated yet", h->device, h->ev, spans, ms2);
}
