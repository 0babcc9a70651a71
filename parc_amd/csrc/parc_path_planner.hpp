// parc_path_planner.hpp — batched terrain path planner on gfx950 (parc_pathplan_*, include/parc_env.h).
//
// Stage 2 of the reference (scripts/parc_2_kin_gen.py:310-337) picks a start and a goal cell near a small terrain's border, simplifies the
// terrain and plans a path with motion_synthesis/procgen/astar.py, one query at a time in Python.  Here Q queries are two launches:
//   k_pp_prepare  one wave per query: the start / goal draw from (seed, query index) with Philox4x32-10 unless the caller injects the
//                 cells (pick_random_start_end_nodes_on_edges :74-97), flat_maxpool_2x2 and the two flatten_4x4_near_edge
//                 (terrain_util.py:1988-2038) in LDS, the simplified heightfield written out
//   k_pp_search   one wave per query, the query's heightfield, g, open-f, parents and cliff flags in LDS: pop the open cell with the
//                 smallest (f, g, cell index), stop at the goal, relax the popped cell's edges across the lanes (8 neighbours, then the
//                 (2R)^2 jump candidates of a cliff cell, 64 per round, each with its Bresenham line-of-sight walk: the jump edges are
//                 formed for popped cells only); then the parents walked back, the node list, the 3-D polyline (:394-441)
//   k_pp_graph    on request (parc_pathplan_get_graph): the same edge predicates for every cell of a range of queries, lane per jump
//                 candidate and one ballot per 64 of them
// A wave per query: no cross-wave reduction in the serial pop loop, throughput comes from the resident queries.  All arithmetic is
// fp32 and unfused in the reference's association; the bumpiness term accumulates its nine fp32 patch sums in double.
// Counters of the generator, key = seed: step-cost noise of edge a -> b of query q: (hi = q, lo = a << 16 | b), first word;
// start / goal draw number t of query q: (hi = 1 << 62 | q, lo = t), words 0 and 1.  q is first_query + the index in the batch, so a
// query computes the same bits alone or in any batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_math.hpp"
#include "parc_tool_handle.hpp"

namespace pplan {
using namespace parc;

constexpr int MAX_DIM = PARC_PATHPLAN_MAX_DIM;
constexpr int MAX_R = PARC_PATHPLAN_MAX_JUMP_RADIUS;
constexpr int JW = PARC_PATHPLAN_JUMP_WORDS;
constexpr unsigned long long DRAW_STREAM = 1ull << 62;
constexpr int MAX_DRAWS = 1000;

struct Cfg {                               // by value
    int X, Y, R, simplify, max_expansions, max_nodes, max_points, use_bumpy;
    float dx, dy, minx, miny;
    float max_z, max_jxy, max_jz, min_jz, w_z, w_xy, noise_w, noise_min, max_cost, draw_thr;
    double w_bumpy, max_bumpy, dxd, split;
};

struct Bufs {
    const float *hf_in;                    // [Q][N]
    float *hf;                             // [Q][N] simplified
    int *start, *goal;                     // [Q][2]
    int *status, *num_nodes, *num_points, *pops, *nodes;
    float *cost, *points;
};

__device__ __forceinline__ float posx(const Cfg &G, int i) { return G.minx + (float)i * G.dx; }   // SubTerrain.get_point (terrain_util.py:193)
__device__ __forceinline__ float posy(const Cfg &G, int j) { return G.miny + (float)j * G.dy; }
__device__ __forceinline__ bool in_ring(int i, int n) { return i == 1 || i == 2 || i == n - 2 || i == n - 3; }

// the k-th cell of the reference's candidate list (rows in order; a ring row holds every column, another row its ring columns)
__device__ int ring_cell(int k, int X, int Y, int ny) {
    for (int i = 0; i < X; ++i) {
        const int cnt = in_ring(i, X) ? Y : ny;
        if (k >= cnt) { k -= cnt; continue; }
        if (in_ring(i, X)) return i * Y + k;
        for (int j = 0; j < Y; ++j)
            if (in_ring(j, Y) && k-- == 0) return i * Y + j;
    }
    return 0;
}

// the Python slice a : a + 4 on an axis of n cells (a negative start counts from the end: idx 0 gives the empty slice(-2, 2) when n > 4)
__device__ __forceinline__ void py_slice4(int idx, int n, int &lo, int &hi) {
    const int a = (idx % 2 == 0) ? idx - 2 : idx - 1;
    lo = a < 0 ? (a + n > 0 ? a + n : 0) : (a < n ? a : n);
    hi = a + 4 < n ? a + 4 : n;
}

__global__ void __launch_bounds__(64) k_pp_prepare(Cfg G, Bufs B, int inject, unsigned long long seed, unsigned long long first_query) {
    extern __shared__ float s_hf[];
    const long long q = blockIdx.x;
    const int lane = threadIdx.x, X = G.X, Y = G.Y, N = X * Y;
    __shared__ int s_sg[2];
    if (lane == 0) {
        int s = 0, g = 0, ok = 1;
        if (inject) {
            s = B.start[2 * q] * Y + B.start[2 * q + 1];
            g = B.goal[2 * q] * Y + B.goal[2 * q + 1];
        } else {
            int nx = 0, ny = 0;
            for (int i = 0; i < X; ++i) nx += in_ring(i, X);
            for (int j = 0; j < Y; ++j) ny += in_ring(j, Y);
            const int n = nx * Y + (X - nx) * ny;
            ok = 0;
            for (int t = 0; t < MAX_DRAWS && !ok; ++t) {
                float u[4];
                philox4(seed, DRAW_STREAM | (first_query + (unsigned long long)q), (unsigned)t, u);
                int a = (int)(u[0] * (float)n), b = (int)(u[1] * (float)n);
                a = a < n - 1 ? a : n - 1; b = b < n - 1 ? b : n - 1;
                s = ring_cell(a, X, Y, ny); g = ring_cell(b, X, Y, ny);
                const float ddx = posx(G, s / Y) - posx(G, g / Y), ddy = posy(G, s % Y) - posy(G, g % Y);
                ok = sqrtf(ddx * ddx + ddy * ddy) >= G.draw_thr;
            }
            B.start[2 * q] = s / Y; B.start[2 * q + 1] = s % Y;
            B.goal[2 * q] = g / Y; B.goal[2 * q + 1] = g % Y;
        }
        B.status[q] = ok ? PARC_PATHPLAN_NO_PATH : PARC_PATHPLAN_NO_DRAW;
        s_sg[0] = s; s_sg[1] = g;
    }
    for (int c = lane; c < N; c += 64) s_hf[c] = B.hf_in[q * N + c];
    __syncthreads();
    if (G.simplify) {
        const int bx = X / 2, by = Y / 2;                    // range(0, dim - 1, 2): the last row / column of an odd grid is left alone
        for (int b = lane; b < bx * by; b += 64) {
            const int i = 2 * (b / by), j = 2 * (b % by);
            const float m = fmaxf(fmaxf(s_hf[i * Y + j], s_hf[i * Y + j + 1]), fmaxf(s_hf[(i + 1) * Y + j], s_hf[(i + 1) * Y + j + 1]));
            s_hf[i * Y + j] = m; s_hf[i * Y + j + 1] = m; s_hf[(i + 1) * Y + j] = m; s_hf[(i + 1) * Y + j + 1] = m;
        }
        __syncthreads();
        for (int k = 0; k < 2; ++k) {                        // the goal's height is read after the start's block is written
            const int c = s_sg[k];
            const float h = s_hf[c];
            int x0, x1, y0, y1;
            py_slice4(c / Y, X, x0, x1);
            py_slice4(c % Y, Y, y0, y1);
            __syncthreads();
            if (lane < 16) {
                const int i = x0 + lane / 4, j = y0 + lane % 4;
                if (i < x1 && j < y1) s_hf[i * Y + j] = h;
            }
            __syncthreads();
        }
    }
    for (int c = lane; c < N; c += 64) B.hf[q * N + c] = s_hf[c];
}

// ---- the navigation graph's predicates (construct_navigation_graph, astar.py:99-205) on a heightfield in LDS ---------------------------
__device__ __forceinline__ bool is_cliff(const float *hf, int i, int j, int X, int Y) {
    if (i == 0 || j == 0 || i == X - 1 || j == Y - 1) return false;
    const float h = hf[i * Y + j];
    return h - hf[(i - 1) * Y + j] > 1e-3f || h - hf[(i + 1) * Y + j] > 1e-3f || h - hf[i * Y + j - 1] > 1e-3f || h - hf[i * Y + j + 1] > 1e-3f;
}

__device__ __forceinline__ bool cliff_bit(const unsigned *bits, int c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

__constant__ int c_dir[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};

__device__ __forceinline__ bool nbr_edge(const Cfg &G, const float *hf, int i, int j, int d) {
    const int r = i + c_dir[d][0], c = j + c_dir[d][1];
    if (r < 0 || r >= G.X || c < 0 || c >= G.Y) return false;
    return fabsf(hf[r * G.Y + c] - hf[i * G.Y + j]) <= G.max_z;
}

// candidate k of the (2R) x (2R) window of cliff cell (i, j): its cell (ii, jj), or false when it is no jump edge
__device__ bool jump_edge(const Cfg &G, const float *hf, const unsigned *cliff, int i, int j, int k, int &ii, int &jj) {
    const int X = G.X, Y = G.Y, R = G.R, W = 2 * R;
    ii = i - R + k / W; jj = j - R + k % W;
    // rows [max(i - R, 1), min(i + R, X - 1)), columns likewise: exclusive upper ends
    if (ii < 1 || ii >= X - 1 || jj < 1 || jj >= Y - 1) return false;
    if (!cliff_bit(cliff, ii * Y + jj)) return false;
    const float ddx = posx(G, i) - posx(G, ii), ddy = posy(G, j) - posy(G, jj);
    if (!(sqrtf(ddx * ddx + ddy * ddy) <= G.max_jxy)) return false;
    const float h0 = hf[i * Y + j], dz = hf[ii * Y + jj] - h0;
    if (!(G.min_jz <= dz && dz <= G.max_jz)) return false;
    const float thr = (h0 + G.max_jz) + 1e-3f;
    // terrain_util.get_line_indices (:1045-1074): Bresenham, both end cells included
    int x0 = i, y0 = j;
    const int adx = abs(ii - i), ady = abs(jj - j), sx = i < ii ? 1 : -1, sy = j < jj ? 1 : -1;
    int err = adx - ady;
    for (int it = 0; it <= adx + ady; ++it) {                // at most adx + ady steps; the bound keeps a broken walk inside the grid
        if (!(hf[x0 * Y + y0] < thr)) return false;
        if (x0 == ii && y0 == jj) return true;
        const int e2 = 2 * err;
        if (e2 > -ady) { err -= ady; x0 += sx; }
        if (e2 < adx) { err += adx; y0 += sy; }
    }
    return false;
}

__device__ void load_query(const Cfg &G, const float *src, float *s_hf, unsigned *s_cliff, int lane) {
    const int X = G.X, Y = G.Y, N = X * Y;
    for (int c = lane; c < N; c += 64) s_hf[c] = src[c];
    __syncthreads();
    for (int w = lane; w < (N + 31) / 32; w += 64) {
        unsigned m = 0u;
        for (int b = 0; b < 32 && w * 32 + b < N; ++b) {
            const int c = w * 32 + b;
            if (is_cliff(s_hf, c / Y, c % Y, X, Y)) m |= 1u << b;
        }
        s_cliff[w] = m;
    }
    __syncthreads();
}

// LDS of k_pp_search: hf, g, open-f [NP] floats each, parents [NP] u16, cliff bits; NP = N rounded up to 256 (one float4 per lane per
// scan round).  16 x 16: 3.6 KB, 64 x 64: 57.9 KB.
__host__ __device__ __forceinline__ int np_of(int N) { return (N + 255) & ~255; }
__host__ __device__ __forceinline__ size_t search_lds(int N) { return (size_t)np_of(N) * 14 + (size_t)((N + 31) / 32) * 4; }

// compute_bumpy_cost (astar.py:237-270), clamped and weighted: nine fp32 patch sums accumulated in double, / 81
__device__ float bumpy_term(const Cfg &G, const float *hf, int i, int j) {
    const int X = G.X, Y = G.Y;
    double mad = 0.0;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b) {
            float s = 0.f;
            for (int u = -1; u <= 1; ++u)
                for (int v = -1; v <= 1; ++v) {
                    const int ci = min(max(i + u, 0), X - 1), cj = min(max(j + v, 0), Y - 1);
                    const int hi = min(max(i + u + a, 0), X - 1), hj = min(max(j + v + b, 0), Y - 1);
                    s = s + fabsf(hf[ci * Y + cj] - hf[hi * Y + hj]);
                }
            mad += (double)s;
        }
    mad = mad / 81;
    if (mad > G.max_bumpy) mad = G.max_bumpy;
    return (float)(mad * G.w_bumpy);
}

// cost() of astar.py:272-295 for the edge c -> t, the noise a pure function of (seed, query, c, t)
__device__ __forceinline__ float step_cost(const Cfg &G, const float *hf, int c, int t, unsigned long long seed, unsigned long long query) {
    const int Y = G.Y, ci = c / Y, cj = c % Y, ti = t / Y, tj = t % Y;
    const float adz = fabsf(hf[t] - hf[c]);
    const float z_cost = (G.w_z * adz) * adz;
    const float xd = posx(G, ti) - posx(G, ci), yd = posy(G, tj) - posy(G, cj);
    const float xy_cost = G.w_xy * (xd * xd + yd * yd);
    float total = xy_cost + z_cost;
    total = total + (G.use_bumpy ? bumpy_term(G, hf, ti, tj) : 0.f);
    float u[4];
    philox4(seed, query, ((unsigned)c << 16) | (unsigned)t, u);
    return total + (u[0] * G.noise_w + G.noise_min);
}

__device__ __forceinline__ float heuristic(const Cfg &G, const float *hf, int t, int goal) {
    const int Y = G.Y;
    const float a = posx(G, t / Y) - posx(G, goal / Y), b = posy(G, t % Y) - posy(G, goal % Y), c = hf[t] - hf[goal];
    return sqrtf((a * a + b * b) + c * c);
}

__device__ __forceinline__ bool key_less(float f, float g, int c, float f2, float g2, int c2) {
    return f < f2 || (f == f2 && (g < g2 || (g == g2 && c < c2)));
}

__global__ void __launch_bounds__(64) k_pp_search(Cfg G, Bufs B, unsigned long long seed, unsigned long long first_query) {
    extern __shared__ float s_mem[];
    const long long q = blockIdx.x;
    const int lane = threadIdx.x, X = G.X, Y = G.Y, N = X * Y, NP = np_of(N);
    float *s_hf = s_mem, *s_g = s_hf + NP, *s_fo = s_g + NP;
    unsigned short *s_par = (unsigned short *)(s_fo + NP);
    unsigned *s_cliff = (unsigned *)(s_par + NP);
    const float inf = __int_as_float(0x7f800000);
    const unsigned long long query = first_query + (unsigned long long)q;
    if (B.status[q] == PARC_PATHPLAN_NO_DRAW) {
        if (lane == 0) { B.cost[q] = __int_as_float(0x7fc00000); B.num_nodes[q] = 0; B.num_points[q] = 0; B.pops[q] = 0; }
        return;
    }
    load_query(G, B.hf + q * N, s_hf, s_cliff, lane);
    for (int c = lane; c < NP; c += 64) { s_g[c] = inf; s_fo[c] = inf; s_par[c] = 0xffffu; }
    __syncthreads();
    const int start = B.start[2 * q] * Y + B.start[2 * q + 1], goal = B.goal[2 * q] * Y + B.goal[2 * q + 1];
    if (lane == 0) { s_g[start] = 0.f; s_fo[start] = 0.f + heuristic(G, s_hf, start, goal); }
    __syncthreads();
    int pops = 0, status = PARC_PATHPLAN_NO_PATH;
    const int W2 = 4 * G.R * G.R;
    for (;;) {
        // pop: the open cell with the smallest (f, g, cell index); a lane scans the float4 groups lane, lane + 64, ...
        float bf = inf, bg = inf;
        int bc = 0x7fffffff;
        for (int v = lane; v < NP / 4; v += 64) {
            const float4 f4 = *(const float4 *)(s_fo + 4 * v);
            const float fs[4] = {f4.x, f4.y, f4.z, f4.w};
            for (int k = 0; k < 4; ++k)
                if (fs[k] <= bf && fs[k] < inf) {
                    const int c = 4 * v + k;
                    const float g = s_g[c];
                    if (key_less(fs[k], g, c, bf, bg, bc)) { bf = fs[k]; bg = g; bc = c; }
                }
        }
        for (int d = 1; d < 64; d <<= 1) {
            const float of = __shfl_xor(bf, d, 64), og = __shfl_xor(bg, d, 64);
            const int oc = __shfl_xor(bc, d, 64);
            if (key_less(of, og, oc, bf, bg, bc)) { bf = of; bg = og; bc = oc; }
        }
        if (bc == 0x7fffffff) break;                          // open set empty: NO_PATH
        if (pops >= G.max_expansions) { status = PARC_PATHPLAN_BUDGET; break; }
        ++pops;
        const int c = bc;
        if (c == goal) { status = PARC_PATHPLAN_FOUND; break; }
        const int ci = c / Y, cj = c % Y;
        const float gc = bg;
        __syncthreads();
        if (lane == 0) s_fo[c] = inf;
        // relax: strict <, an unseen cell is +inf.  Targets of one round are distinct cells; a jump edge onto an adjacent cell repeats
        // a neighbour edge with the same cost (the noise is a function of the edge), so the second evaluation changes nothing
        const bool cl = cliff_bit(s_cliff, c);
        for (int base = -64; base < (cl ? W2 : 0); base += 64) {     // round -64: the neighbours; the trip count is wave-uniform
            const int k = base + lane;
            int t = -1;
            if (k < 0) {
                const int d = k + 64;
                if (d < 8 && nbr_edge(G, s_hf, ci, cj, d)) t = (ci + c_dir[d][0]) * Y + cj + c_dir[d][1];
            } else if (k < W2) {
                int ii, jj;
                if (jump_edge(G, s_hf, s_cliff, ci, cj, k, ii, jj)) t = ii * Y + jj;
            }
            if (t >= 0) {
                const float tg = gc + step_cost(G, s_hf, c, t, seed, query);
                if (tg < s_g[t]) { s_g[t] = tg; s_fo[t] = tg + heuristic(G, s_hf, t, goal); s_par[t] = (unsigned short)c; }
            }
            __syncthreads();
        }
        __syncthreads();
    }
    __syncthreads();
    if (lane != 0) return;
    // run_a_star_on_start_end_nodes (astar.py:394-441), one lane: a path is a few dozen cells
    B.pops[q] = pops;
    float cost = __int_as_float(0x7fc00000);
    int nn = 0, np = 0;
    if (status == PARC_PATHPLAN_FOUND) {
        cost = s_g[goal];
        if (cost > G.max_cost) status = PARC_PATHPLAN_OVER_MAX_COST;
        for (int c = goal; c != start && nn < N; c = s_par[c]) ++nn;
        ++nn;
        int *nodes = B.nodes + q * G.max_nodes;
        int k = nn - 1;
        for (int c = goal; k >= 0; c = s_par[c], --k) {
            if (k < G.max_nodes) nodes[k] = c;
            if (c == start) break;
        }
        if (status == PARC_PATHPLAN_FOUND && nn <= G.max_nodes) {
            float *pts = B.points + q * G.max_points * 3;
            float px = 0.f, py = 0.f, pz = 0.f;
            for (k = 0; k < nn; ++k) {
                const int c = nodes[k];
                const float x = posx(G, c / Y), y = posy(G, c % Y), z = s_hf[c];
                const float xd = x - px, yd = y - py;
                const double dist = (double)sqrtf(xd * xd + yd * yd);
                if (k > 0 && dist > G.split) {
                    // torch.linspace(prev, cur, steps)[1:], steps = ceil(xy_dist / dx) in double on the fp32 operands
                    const int steps = (int)ceil(dist / G.dxd);
                    const float sx = (x - px) / (float)(steps - 1), sy = (y - py) / (float)(steps - 1), sz = (z - pz) / (float)(steps - 1);
                    for (int n = 1; n < steps; ++n, ++np) {
                        if (np >= G.max_points) continue;
                        const bool first = n < steps / 2;
                        const float m = (float)(first ? n : steps - n - 1);
                        pts[3 * np] = first ? px + sx * m : x - sx * m;
                        pts[3 * np + 1] = first ? py + sy * m : y - sy * m;
                        pts[3 * np + 2] = first ? pz + sz * m : z - sz * m;
                    }
                } else {
                    if (np < G.max_points) { pts[3 * np] = x; pts[3 * np + 1] = y; pts[3 * np + 2] = z; }
                    ++np;
                }
                px = x; py = y; pz = z;
            }
        }
    }
    B.status[q] = status; B.cost[q] = cost; B.num_nodes[q] = nn; B.num_points[q] = np;
}

// the graph of queries [q0, q0 + gridDim.x): nbr [n][N] the 8-neighbour mask (bit d = direction d of astar.py:112), cliff [n][N],
// jump [n][N][JW] one bit per window candidate (bit k = row k / 2R, column k % 2R of the window whose corner is (i - R, j - R))
__global__ void __launch_bounds__(64) k_pp_graph(Cfg G, const float *hf, int q0, unsigned char *nbr, unsigned char *cliff, unsigned *jump) {
    extern __shared__ float s_mem[];
    const int lane = threadIdx.x, X = G.X, Y = G.Y, N = X * Y;
    float *s_hf = s_mem;
    unsigned *s_cliff = (unsigned *)(s_hf + N);
    const long long o = blockIdx.x;
    load_query(G, hf + ((long long)q0 + o) * N, s_hf, s_cliff, lane);
    for (int c = lane; c < N; c += 64) {
        unsigned m = 0u;
        for (int d = 0; d < 8; ++d) m |= nbr_edge(G, s_hf, c / Y, c % Y, d) ? 1u << d : 0u;
        nbr[o * N + c] = (unsigned char)m;
        cliff[o * N + c] = cliff_bit(s_cliff, c) ? 1 : 0;
    }
    const int W2 = 4 * G.R * G.R;
    for (int c = 0; c < N; ++c) {
        const bool cl = cliff_bit(s_cliff, c);
        for (int r = 0; r < JW / 2; ++r) {
            const int k = r * 64 + lane;
            int ii, jj;
            const bool e = cl && k < W2 && jump_edge(G, s_hf, s_cliff, c / Y, c % Y, k, ii, jj);
            const unsigned long long b = __ballot(e);
            if (lane == 0) { jump[(o * N + c) * JW + 2 * r] = (unsigned)b; jump[(o * N + c) * JW + 2 * r + 1] = (unsigned)(b >> 32); }
        }
    }
}

}  // namespace pplan

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------
struct ParcPathPlanner : tool::Handle<DeviceEvents<3>> {   // mem: unused, the buffers are the batch's
    struct Batch {                        // the buffers of up to cap queries; they exist once the handle holds one
        DeviceArena mem;
        pplan::Bufs B{};
        int cap = 0, last_q = 0;          // last_q: queries of the last completed run (0 = none), what parc_pathplan_get_graph may read
    };
    pplan::Cfg cfg{};
    std::unique_ptr<Batch> batch;
    float graph_ms = 0.f;
    bool timed = false;
};

extern "C" void parc_pathplan_destroy(ParcPathPlanner *h) { tool::destroy(h); }

extern "C" int parc_pathplan_create(const ParcPathPlanParams *p, ParcPathPlanner **out) {
    PARC_TRY(tool::create_args("pathplan", "ParcPathPlanParams", p, out));
    if (p->dim_x < 4 || p->dim_y < 4 || p->dim_x > PARC_PATHPLAN_MAX_DIM || p->dim_y > PARC_PATHPLAN_MAX_DIM)
        return fail(PARC_ERR_INVALID, "pathplan: the grid is " + std::to_string(p->dim_x) + " x " + std::to_string(p->dim_y) + ", the planner takes 4 .. " +
                                          std::to_string(PARC_PATHPLAN_MAX_DIM) + " cells a side (PARC_PATHPLAN_MAX_DIM: a query's search state lives in LDS)");
    if (!(p->dx > 0.f) || !(p->dy > 0.f)) return fail(PARC_ERR_INVALID, "pathplan: dx and dy must be > 0");
    if (!(p->max_jump_xy_dist >= 0.0)) return fail(PARC_ERR_INVALID, "pathplan: max_jump_xy_dist must be >= 0");
    const double rr = ceil(p->max_jump_xy_dist / (double)p->dx);     // np.ceil(max_jump_xy_dist / dxdy[0].item())
    if (rr > PARC_PATHPLAN_MAX_JUMP_RADIUS)
        return fail(PARC_ERR_INVALID, "pathplan: max_jump_xy_dist / dx gives a jump window radius of " + std::to_string((long long)rr) + " cells, above the limit of " +
                                          std::to_string(PARC_PATHPLAN_MAX_JUMP_RADIUS) + " (PARC_PATHPLAN_MAX_JUMP_RADIUS)");
    if (p->max_expansions < 1 || p->max_nodes < 1 || p->max_points < 1) return fail(PARC_ERR_INVALID, "pathplan: max_expansions, max_nodes and max_points must be >= 1");
    return tool::create("pathplan", p->device, out, [&](ParcPathPlanner &h) -> int {
        pplan::Cfg &G = h.cfg;
        G.X = p->dim_x; G.Y = p->dim_y; G.R = (int)rr; G.simplify = p->simplify_terrain; G.max_expansions = p->max_expansions;
        G.max_nodes = p->max_nodes; G.max_points = p->max_points; G.use_bumpy = p->w_bumpy != 0.0;
        G.dx = p->dx; G.dy = p->dy; G.minx = p->min_point[0]; G.miny = p->min_point[1];
        // the reference compares and multiplies its Python-float settings as fp32 weak scalars
        G.max_z = (float)p->max_z_diff; G.max_jxy = (float)p->max_jump_xy_dist; G.max_jz = (float)p->max_jump_z_diff; G.min_jz = (float)p->min_jump_z_diff;
        G.w_z = (float)p->w_z; G.w_xy = (float)p->w_xy; G.noise_w = (float)(p->uniform_cost_max - p->uniform_cost_min); G.noise_min = (float)p->uniform_cost_min;
        G.max_cost = (float)p->max_cost; G.draw_thr = (float)(p->min_start_end_xy_dist - 1e-4);
        G.w_bumpy = p->w_bumpy; G.max_bumpy = p->max_bumpy; G.dxd = (double)p->dx;
        G.split = sqrt((double)p->dx * (double)p->dx + (double)p->dy * (double)p->dy) + 1e-3;
        PARC_TRY(h.ev.create());
        if (hipFuncSetAttribute((const void *)pplan::k_pp_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pplan::search_lds(G.X * G.Y)) != hipSuccess)
            return fail(PARC_ERR_HIP, "pathplan: the search kernel's LDS request was refused");
        return PARC_OK;
    });
}

// Buffers for Q queries: kept while they are large enough; otherwise the old ones are released first, the new ones built in a local and
// installed last, so a failed allocation leaves the handle without buffers (and without a last batch), never with some of them.
static int pplan_reserve(ParcPathPlanner *h, int Q) {
    if (h->batch && Q <= h->batch->cap) return PARC_OK;
    std::unique_ptr<ParcPathPlanner::Batch> nb;
    PARC_TRY(tool::renew("pathplan", h->batch, nb));
    const pplan::Cfg &G = h->cfg;
    const long long N = (long long)G.X * G.Y;
    pplan::Bufs &B = nb->B;
    DeviceArena &mem = nb->mem;
    PARC_TRY(mem.alloc(B.hf_in, Q * N));
    PARC_TRY(mem.alloc(B.hf, Q * N));
    PARC_TRY(mem.alloc(B.start, 2LL * Q)); PARC_TRY(mem.alloc(B.goal, 2LL * Q));
    PARC_TRY(mem.alloc(B.status, Q)); PARC_TRY(mem.alloc(B.num_nodes, Q)); PARC_TRY(mem.alloc(B.num_points, Q)); PARC_TRY(mem.alloc(B.pops, Q));
    PARC_TRY(mem.alloc(B.nodes, (long long)Q * G.max_nodes));
    PARC_TRY(mem.alloc(B.cost, Q));
    PARC_TRY(mem.alloc(B.points, (long long)Q * G.max_points * 3));
    nb->cap = Q;
    h->batch = std::move(nb);
    return PARC_OK;
}

extern "C" int parc_pathplan_run(ParcPathPlanner *h, int32_t Q, const float *hf_host, const int32_t *start_host, const int32_t *goal_host, uint64_t seed,
                                 uint64_t first_query, const ParcPathPlanOutputs *out) {
    if (!h || !hf_host || !out) return fail(PARC_ERR_INVALID, "pathplan: null argument");
    if (Q < 1) return fail(PARC_ERR_INVALID, "pathplan: the batch must hold at least one query");
    if ((start_host == nullptr) != (goal_host == nullptr)) return fail(PARC_ERR_INVALID, "pathplan: start and goal cells go together");
    const pplan::Cfg &G = h->cfg;
    const long long N = (long long)G.X * G.Y;
    if (start_host)
        for (long long i = 0; i < 2LL * Q; ++i) {
            const int lim = (i & 1) ? G.Y : G.X;
            if (start_host[i] < 0 || start_host[i] >= lim || goal_host[i] < 0 || goal_host[i] >= lim)
                return fail(PARC_ERR_INVALID, "pathplan: a start / goal cell of query " + std::to_string(i / 2) + " lies outside the grid");
        }
    HIPCHK(hipSetDevice(h->device));
    if (int rc = pplan_reserve(h, Q)) return rc;
    h->batch->last_q = 0;
    const pplan::Bufs &B = h->batch->B;
    HIPCHK(hipMemcpy((void *)B.hf_in, hf_host, (size_t)(Q * N) * sizeof(float), hipMemcpyHostToDevice));
    if (start_host) {
        HIPCHK(hipMemcpy(B.start, start_host, (size_t)Q * 2 * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(B.goal, goal_host, (size_t)Q * 2 * sizeof(int), hipMemcpyHostToDevice));
    }
    HIPCHK(hipEventRecord(h->ev[0], 0));
    PARC_TRY(tool::launch(pplan::k_pp_prepare, dim3((unsigned)Q), dim3(64), (size_t)N * sizeof(float), 0, G, B, start_host ? 1 : 0, (unsigned long long)seed,
                       (unsigned long long)first_query));
    HIPCHK(hipEventRecord(h->ev[1], 0));
    PARC_TRY(tool::launch(pplan::k_pp_search, dim3((unsigned)Q), dim3(64), pplan::search_lds((int)N), 0, G, B, (unsigned long long)seed,
                       (unsigned long long)first_query));
    HIPCHK(hipEventRecord(h->ev[2], 0));
    HIPCHK(hipEventSynchronize(h->ev[2]));
    h->timed = true;
    h->batch->last_q = Q;
    const size_t q = (size_t)Q;
    if (out->status) HIPCHK(hipMemcpy(out->status, B.status, q * sizeof(int), hipMemcpyDeviceToHost));
    if (out->cost) HIPCHK(hipMemcpy(out->cost, B.cost, q * sizeof(float), hipMemcpyDeviceToHost));
    if (out->num_nodes) HIPCHK(hipMemcpy(out->num_nodes, B.num_nodes, q * sizeof(int), hipMemcpyDeviceToHost));
    if (out->nodes) HIPCHK(hipMemcpy(out->nodes, B.nodes, q * G.max_nodes * sizeof(int), hipMemcpyDeviceToHost));
    if (out->num_points) HIPCHK(hipMemcpy(out->num_points, B.num_points, q * sizeof(int), hipMemcpyDeviceToHost));
    if (out->points) HIPCHK(hipMemcpy(out->points, B.points, q * G.max_points * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->start) HIPCHK(hipMemcpy(out->start, B.start, q * 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (out->goal) HIPCHK(hipMemcpy(out->goal, B.goal, q * 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (out->hf) HIPCHK(hipMemcpy(out->hf, B.hf, q * N * sizeof(float), hipMemcpyDeviceToHost));
    if (out->pops) HIPCHK(hipMemcpy(out->pops, B.pops, q * sizeof(int), hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_pathplan_get_graph(ParcPathPlanner *h, int32_t q0, int32_t n, uint8_t *nbr_host, uint8_t *cliff_host, uint32_t *jump_host) {
    if (!h || !nbr_host || !cliff_host || !jump_host) return fail(PARC_ERR_INVALID, "pathplan: null argument");
    if (!h->batch || h->batch->last_q == 0) return fail(PARC_ERR_STATE, "pathplan: parc_pathplan_run first");
    if (q0 < 0 || n < 1 || (long long)q0 + n > h->batch->last_q) return fail(PARC_ERR_INVALID, "pathplan: the query range lies outside the last batch");
    HIPCHK(hipSetDevice(h->device));
    const pplan::Cfg &G = h->cfg;
    const long long cells = (long long)n * G.X * G.Y;
    DeviceArena tmp;                      // this call's outputs and its two events
    DeviceEvents<2> t;
    unsigned char *d_nbr = nullptr, *d_cliff = nullptr;
    unsigned *d_jump = nullptr;
    PARC_TRY(tmp.alloc(d_nbr, cells));
    PARC_TRY(tmp.alloc(d_cliff, cells));
    PARC_TRY(tmp.alloc(d_jump, cells * PARC_PATHPLAN_JUMP_WORDS));
    PARC_TRY(t.create());
    HIPCHK(hipEventRecord(t[0], 0));
    PARC_TRY(tool::launch(pplan::k_pp_graph, dim3((unsigned)n), dim3(64), (size_t)G.X * G.Y * sizeof(float) + (size_t)((G.X * G.Y + 31) / 32) * 4, 0, G, h->batch->B.hf,
                       (int)q0, d_nbr, d_cliff, d_jump));
    HIPCHK(hipEventRecord(t[1], 0));
    HIPCHK(hipMemcpy(nbr_host, d_nbr, (size_t)cells, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cliff_host, d_cliff, (size_t)cells, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(jump_host, d_jump, (size_t)cells * PARC_PATHPLAN_JUMP_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost));
    return t.elapsed(h->graph_ms, 0, 1);
}

extern "C" int parc_pathplan_kernel_times(ParcPathPlanner *h, float *ms3) {
    if (!h || !ms3) return fail(PARC_ERR_INVALID, "pathplan: null argument");
    const tool::Span spans[] = {{h->timed, 0, 1}, {h->timed, 1, 2}};   // prepare, search
    PARC_TRY(tool::span_times("pathplan: nothing planned yet", h->device, h->ev, spans, ms3));
    ms3[2] = h->graph_ms;
    return PARC_OK;
}
