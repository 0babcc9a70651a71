// parc_render_scene.hpp — scene render (parc_env_render_scene): one image of the terrain and the characters of many envs, every
// character at state + env_offsets in the one world, as the reference's viewer draws the whole sim (ig_parkour_env.py:409-441).
// On top of parc_render.hpp, whose camera, terrain DDA and intersection functions it reuses unchanged.
//
// Launch sequence (all on the caller's stream, no host sync; `slot` = one character: list entry i, kind 0 simulated / 1 reference):
//   k_scene_init     1 block: zero the bin counters, reset the reductions, the pose-independent radius of a character about its root.
//   k_scene_roots    per slot: env id in [0, N) and a finite root, else the slot is dropped; the root in the camera-target frame;
//                    lowest root - radius (the floor of the shadow-caster cull).
//   k_scene_prep     per slot: view cull on the root + pose-independent radius; a character whose shadow can reach the view is kept
//                    (its sphere swept along -sun down to the lowest receiver).  FK of the survivors (joint_dof_to_rot, fk_thread)
//                    into the slot's record (body rotations + positions, camera-target frame), the tight bounding sphere exactly as
//                    k_render forms it, and the bounding box / largest radius of the survivors (atomicMin / atomicMax on ordered ints).
//   k_scene_count    per slot: +1 on every bin the sphere overlaps.  Uniform xy grid over the box, at most 64 x 64 bins, bin edge at
//                    least twice the largest radius, so a sphere overlaps at most 2 x 2 bins and the item list is 4 per slot.
//   k_scene_scan     1 block: exclusive scan of the counts.
//   k_scene_scatter  per slot: the slot into each of its bins (atomicAdd on the bin's cursor).
//   k_render_scene   the k_render tile shape (16 x 16 pixels, 256 threads): terrain DDA as k_render, then a 2-D DDA over the bins; in a
//                    bin every character's sphere, then its primitives, formed from the record and the LDS copy of RenderGeoms.  Shadow
//                    rays take the same traversal.
// Order independence: a hit replaces the best one when t is smaller, or t is equal and (env, kind, geom) is smaller; the terrain wins
// ties as in k_render.  The walk stops once the next bin starts beyond the best t, so the result is the minimum over every character
// that can reach it whatever order the atomics filled the bins in.  Every loop is bounded by a count.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/parc_env.h"
#include "parc_env_ops.hpp"      // fk_thread
#include "parc_env_tables.hpp"   // DevTables, joint_dof_to_rot
#include "parc_math.hpp"
#include "parc_render.hpp"       // RenderArgs, RenderGeoms, the camera, the terrain DDA, the primitive intersections

#define SCENE_BINS_SIDE 64
#define SCENE_MAX_BINS (SCENE_BINS_SIDE * SCENE_BINS_SIDE)
#define SCENE_BINS_PER_SLOT 4
#define SCENE_MAX_COORD 1.0e5f   // a root farther than 100 km from the camera target is dropped (a broken state, not a scene)

struct SceneHdr {       // reductions of one call; floats as ordered ints (scene_key)
    int lo[3], hi[3];   // box of the surviving bounding spheres
    int rmax;           // largest surviving radius
    int zlow;           // lowest valid root - rchar
    float rchar;        // pose-independent bound of a character about its root (k_scene_init)
    int pad[7];
};

struct SceneArgs {
    RenderArgs R;               // camera, state, terrain and rgba / depth / id exactly as for k_render; R.env_ids = the draw list
    int n, nk, cam_env, stride; // list length, characters per env (1, 2 with draw_ref), camera env, floats per record
    float hmin;                 // lowest column top (world)
    int *env_map;
    float *rec;                 // [slots][stride]: body rotations (4 B floats), then body positions (3 B floats)
    float4 *sph;                // [slots] root (k_scene_roots), then the bounding sphere (k_scene_prep)
    int *skey;                  // [slots] 2 env + kind, -1 = not drawn
    int *items;                 // [4 slots]
    int *bin_count, *bin_start, *bin_cursor; // [SCENE_MAX_BINS], [SCENE_MAX_BINS + 1], [SCENE_MAX_BINS]
    SceneHdr *hdr;
};

struct SceneGrid { float x0, y0, s, z0, z1; int nx, ny; };

struct SceneFrame { V3 t_loc, eoc, eye, f, rt, up; };

__device__ __forceinline__ int scene_key(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float scene_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
__device__ __forceinline__ bool finite3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// The camera of k_render, for the camera env: target frame origin, eye and basis (the same arithmetic, so the camera env's own scene
// render forms the same rays).
__device__ __forceinline__ SceneFrame scene_frame(const RenderArgs &A, int c) {
    SceneFrame F;
    const V3 root = r_ld(A.root_pos + 3 * (size_t)c);
    F.eoc = r_ld(A.env_off + 3 * (size_t)c);
    F.t_loc = A.cam_mode == 0 ? root : r_ld(A.tgt);
    F.eye = A.cam_mode == 0 ? r_ld(A.off) : r_sub(r_ld(A.eye), F.t_loc);
    F.f = normalize3(r_mul(F.eye, -1.f));
    V3 rt = cross3(F.f, mk3(0.f, 0.f, 1.f));
    if (norm3(rt) < 1e-6f) rt = cross3(F.f, mk3(0.f, 1.f, 0.f));
    F.rt = normalize3(rt);
    F.up = cross3(F.rt, F.f);
    return F;
}

// Root of slot (e, kind) in the camera-target frame: (root - t_loc) + (env origin - camera env origin).  For the camera env the second
// term is exactly 0, so its characters get the very root k_render passes to fk_thread.
__device__ __forceinline__ V3 scene_root(const RenderArgs &A, const SceneFrame &F, int e, int kind) {
    const V3 d = r_sub(r_ld(A.env_off + 3 * (size_t)e), F.eoc);
    V3 p;
    if (kind == 0) p = r_sub(r_ld(A.root_pos + 3 * (size_t)e), F.t_loc);
    else {
        const float *rp = A.ref_root_pos + 3 * (size_t)e;
        p = mk3(rp[0] + A.ref_off[0] - F.t_loc.x, rp[1] + A.ref_off[1] - F.t_loc.y, rp[2] + A.ref_off[2] - F.t_loc.z);
    }
    return r_add(p, d);
}

__device__ __forceinline__ SceneGrid scene_grid(const SceneHdr *h) {
    SceneGrid g;
    const float lx = scene_unkey(h->lo[0]), ly = scene_unkey(h->lo[1]), hx = scene_unkey(h->hi[0]), hy = scene_unkey(h->hi[1]);
    if (!(lx <= hx)) { g.x0 = g.y0 = g.z0 = g.z1 = 0.f; g.s = 1.f; g.nx = g.ny = 0; return g; }   // nothing survived
    const float pad = 1e-3f;
    g.x0 = lx - pad; g.y0 = ly - pad;
    g.z0 = scene_unkey(h->lo[2]) - pad; g.z1 = scene_unkey(h->hi[2]) + pad;
    const float wx = hx - lx + 2.f * pad, wy = hy - ly + 2.f * pad;
    g.s = fmaxf(fmaxf(2.f * scene_unkey(h->rmax) * 1.001f, 1e-2f), fmaxf(wx, wy) * (1.0001f / SCENE_BINS_SIDE));
    g.nx = min(max((int)ceilf(wx / g.s), 1), SCENE_BINS_SIDE);
    g.ny = min(max((int)ceilf(wy / g.s), 1), SCENE_BINS_SIDE);
    return g;
}

// Bins [i0, i1] x [j0, j1] of a sphere: at most 2 x 2 (the bin edge is at least the diameter; the clamp keeps the bound under rounding).
__device__ __forceinline__ void scene_bins(const SceneGrid &g, float4 sp, int &i0, int &i1, int &j0, int &j1) {
    i0 = min(max((int)floorf((sp.x - sp.w - g.x0) / g.s), 0), g.nx - 1);
    i1 = min(max((int)floorf((sp.x + sp.w - g.x0) / g.s), i0), min(i0 + 1, g.nx - 1));
    j0 = min(max((int)floorf((sp.y - sp.w - g.y0) / g.s), 0), g.ny - 1);
    j1 = min(max((int)floorf((sp.y + sp.w - g.y0) / g.s), j0), min(j0 + 1, g.ny - 1));
}

__global__ __launch_bounds__(256) void k_scene_init(const SceneArgs S) {
    for (int b = threadIdx.x; b < SCENE_MAX_BINS; b += blockDim.x) S.bin_count[b] = 0;
    if (threadIdx.x == 0) {
        SceneHdr &h = *S.hdr;
        for (int c = 0; c < 3; ++c) { h.lo[c] = scene_key(__int_as_float(0x7f800000)); h.hi[c] = scene_key(__int_as_float(0xff800000)); }
        h.rmax = 0;
        h.zlow = scene_key(__int_as_float(0x7f800000));
        // farthest point of any pose from the root: chain of link lengths to the body + the geom's reach in its body + its extent
        const DevTables *T = S.R.tables;
        const RenderGeoms &G = *S.R.geoms;
        float dist[PARC_MAX_BODIES];
        dist[0] = 0.f;
        for (int j = 1; j < S.R.B; ++j) {
            const int p = T->h.parent[j];
            dist[j] = (p >= 0 && p < j ? dist[p] : 0.f) + norm3(mk3(T->h.lt[j][0], T->h.lt[j][1], T->h.lt[j][2]));
        }
        float r = 0.f;
        for (int g = 0; g < G.n; ++g) {
            const float ext = G.type[g] == PARC_GEOM_BOX ? norm3(r_ld(G.size[g])) : G.size[g][0];
            const float reach = fmaxf(norm3(r_ld(G.p0[g])), G.type[g] == PARC_GEOM_CAPSULE ? norm3(r_ld(G.p1[g])) : 0.f);
            r = fmaxf(r, dist[G.body[g]] + reach + ext);
        }
        h.rchar = r * 1.001f + 1e-3f;
    }
}

__global__ __launch_bounds__(256) void k_scene_roots(const SceneArgs S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.n * S.nk) return;
    const int i = s / S.nk, kind = s - i * S.nk;
    const long long ev = S.R.env_ids ? (long long)S.R.env_ids[i] : (long long)i;
    int key = -1;
    if (ev >= 0 && ev < S.R.N) {                                    // ids outside [0, N) are skipped, never dereferenced
        const int e = (int)ev;
        const SceneFrame F = scene_frame(S.R, S.cam_env);
        const V3 c = scene_root(S.R, F, e, kind);
        if (finite3(c) && fabsf(c.x) < SCENE_MAX_COORD && fabsf(c.y) < SCENE_MAX_COORD && fabsf(c.z) < SCENE_MAX_COORD) {
            key = 2 * e + kind;
            S.sph[s] = make_float4(c.x, c.y, c.z, 0.f);
            atomicMin(&S.hdr->zlow, scene_key(c.z - S.hdr->rchar));
        }
    }
    S.skey[s] = key;
}

// Is the swept sphere (segment v0 -> v1, radius R, eye-relative) entirely outside one of the view's five planes?
__device__ __forceinline__ bool scene_outside(const SceneFrame &F, float tx, float ty, V3 v0, V3 v1, float R) {
    const float ax = rsqrtf(tx * tx + 1.f), ay = rsqrtf(ty * ty + 1.f);
    const V3 n[5] = {F.f,
                     r_mul(r_sub(r_mul(F.f, tx), F.rt), ax), r_mul(r_add(r_mul(F.f, tx), F.rt), ax),
                     r_mul(r_sub(r_mul(F.f, ty), F.up), ay), r_mul(r_add(r_mul(F.f, ty), F.up), ay)};
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (r_dot(n[k], v0) < -R && r_dot(n[k], v1) < -R) return true;
    return false;
}

__global__ __launch_bounds__(64) void k_scene_prep(const SceneArgs S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.n * S.nk) return;
    const int key = S.skey[s];
    if (key < 0) return;
    const RenderArgs &A = S.R;
    const int e = key >> 1, kind = key & 1, B = A.B;
    const SceneFrame F = scene_frame(A, S.cam_env);
    const float4 s0 = S.sph[s];
    const V3 c = mk3(s0.x, s0.y, s0.z);
    // ---- cull on the root + the pose-independent radius, before any FK ----
    const float R = S.hdr->rchar * 1.01f + 1e-2f;
    const V3 v0 = r_sub(c, F.eye);
    bool keep = true;
    if (!A.shadows) keep = !scene_outside(F, A.tan_half * A.aspect, A.tan_half, v0, v0, R);
    else if (A.sun[2] > 1e-3f) {
        // the shadow of the sphere lies along -sun; receivers sit no lower than the lowest column top or the lowest character
        const float zfloor = fminf(S.hmin - (F.t_loc.z + F.eoc.z), scene_unkey(S.hdr->zlow));
        const float sm = fmaxf((c.z + R - zfloor) / A.sun[2], 0.f);
        keep = !scene_outside(F, A.tan_half * A.aspect, A.tan_half, v0, r_sub(v0, r_mul(r_ld(A.sun), sm)), R);
    } // sun at or below the horizon: shadows run without end, every character is kept
    if (!keep) { S.skey[s] = -1; return; }
    // ---- FK into the record ----
    float jr[4 * (PARC_MAX_BODIES - 1)];
    for (int j = 1; j < B; ++j) {
        const Q4 q = kind == 0 ? joint_dof_to_rot(A.tables->h.jtype[j], A.tables->h.axis[j], A.dof_pos + (size_t)A.D * e + A.tables->h.dof_idx[j])
                               : *(const float4 *)(A.ref_joint_rot + 4 * ((size_t)e * (B - 1) + j - 1));
        *(float4 *)(jr + 4 * (j - 1)) = q;
    }
    float *rec = S.rec + (size_t)s * S.stride;
    const float *rr = (kind == 0 ? A.root_rot : A.ref_root_rot) + 4 * (size_t)e;
    fk_thread(A.tables, B, c, mk4(rr[0], rr[1], rr[2], rr[3]), jr, rec + 4 * B, rec);
    // ---- the bounding sphere of k_render (same arithmetic) ----
    const RenderGeoms &G = *A.geoms;
    float r = 0.f;
    for (int g = 0; g < G.n; ++g) {
        const int b = G.body[g];
        const Q4 q = *(const float4 *)(rec + 4 * b);
        const V3 bp = r_ld(rec + 4 * B + 3 * b);
        const V3 a = r_add(bp, quat_rotate(q, r_ld(G.p0[g])));
        const V3 bb = G.type[g] == PARC_GEOM_CAPSULE ? r_add(bp, quat_rotate(q, r_ld(G.p1[g]))) : a;
        const float ext = G.type[g] == PARC_GEOM_BOX ? sqrtf(G.size[g][0] * G.size[g][0] + G.size[g][1] * G.size[g][1] + G.size[g][2] * G.size[g][2])
                                                     : G.size[g][0];
        r = fmaxf(r, fmaxf(norm3(r_sub(a, c)), norm3(r_sub(bb, c))) + ext);
    }
    const float rad = r * 1.0001f + 1e-4f;
    if (!(rad < SCENE_MAX_COORD)) { S.skey[s] = -1; return; }      // NaN / runaway rotations: not drawn
    S.sph[s] = make_float4(c.x, c.y, c.z, rad);
    atomicMin(&S.hdr->lo[0], scene_key(c.x - rad)); atomicMin(&S.hdr->lo[1], scene_key(c.y - rad)); atomicMin(&S.hdr->lo[2], scene_key(c.z - rad));
    atomicMax(&S.hdr->hi[0], scene_key(c.x + rad)); atomicMax(&S.hdr->hi[1], scene_key(c.y + rad)); atomicMax(&S.hdr->hi[2], scene_key(c.z + rad));
    atomicMax(&S.hdr->rmax, scene_key(rad));
}

__global__ __launch_bounds__(256) void k_scene_count(const SceneArgs S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.n * S.nk || S.skey[s] < 0) return;
    const SceneGrid g = scene_grid(S.hdr);
    int i0, i1, j0, j1;
    scene_bins(g, S.sph[s], i0, i1, j0, j1);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) atomicAdd(&S.bin_count[j * g.nx + i], 1);
}

__global__ __launch_bounds__(1024) void k_scene_scan(const SceneArgs S) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, per = SCENE_MAX_BINS / 1024;
    int v[SCENE_MAX_BINS / 1024], sum = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) { v[k] = S.bin_count[tid * per + k]; sum += v[k]; }
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int t = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    int run = part[tid] - sum;
#pragma unroll
    for (int k = 0; k < per; ++k) { S.bin_start[tid * per + k] = run; S.bin_cursor[tid * per + k] = run; run += v[k]; }
    if (tid == 1023) S.bin_start[SCENE_MAX_BINS] = run;
}

__global__ __launch_bounds__(256) void k_scene_scatter(const SceneArgs S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.n * S.nk || S.skey[s] < 0) return;
    const SceneGrid g = scene_grid(S.hdr);
    int i0, i1, j0, j1;
    scene_bins(g, S.sph[s], i0, i1, j0, j1);
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) S.items[atomicAdd(&S.bin_cursor[j * g.nx + i], 1)] = s;
}

struct SHit { int key, slot; };   // 2 env + kind of the best character hit (INT_MAX: none) and its slot

// The characters along O + t d, t in [0, tmax), over the bins.  h holds the best hit so far (the terrain's, or none); ANY: the first
// hit ends the walk (shadow rays).
template <bool ANY>
__device__ bool scene_chars(const SceneArgs &S, const RenderGeoms &G, const SceneGrid &g, V3 O, V3 d, float tmax, RHit &h, SHit &sh) {
    if (g.nx == 0) return false;
    const float inf = RENDER_NO_HIT;
    const float ix = d.x != 0.f ? 1.f / d.x : inf, iy = d.y != 0.f ? 1.f / d.y : inf;
    float t0 = 0.f, t1 = tmax;
    const float lo[3] = {g.x0, g.y0, g.z0}, hi[3] = {g.x0 + g.nx * g.s, g.y0 + g.ny * g.s, g.z1};
    const float o[3] = {O.x, O.y, O.z}, dd[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dd[k] != 0.f) {
            const float inv = 1.f / dd[k];
            const float ta = (lo[k] - o[k]) * inv, tb = (hi[k] - o[k]) * inv;
            t0 = fmaxf(t0, fminf(ta, tb)); t1 = fminf(t1, fmaxf(ta, tb));
        } else if (o[k] < lo[k] || o[k] > hi[k]) return false;
    }
    if (!(t0 <= t1)) return false;
    const V3 P = r_add(O, r_mul(d, t0));
    int i = min(max((int)floorf((P.x - g.x0) / g.s), 0), g.nx - 1), j = min(max((int)floorf((P.y - g.y0) / g.s), 0), g.ny - 1);
    const int sx = d.x > 0.f ? 1 : -1, sy = d.y > 0.f ? 1 : -1;
    const int max_steps = g.nx + g.ny + 2;
    bool hit = false;
    for (int it = 0; it < max_steps; ++it) {
        const int b = j * g.nx + i;
        const int k1 = S.bin_start[b + 1];
        for (int k = S.bin_start[b]; k < k1; ++k) {
            const int slot = S.items[k];
            const float4 sp = S.sph[slot];
            const V3 oc = r_sub(O, mk3(sp.x, sp.y, sp.z));
            const float bq = r_dot(oc, d), cc = r_dot(oc, oc) - sp.w * sp.w, disc = bq * bq - cc;
            if (disc < 0.f || (bq > 0.f && cc > 0.f)) continue;      // the bounding-sphere test of chars_hit
            if (-bq - sqrtf(disc) > fminf(h.t, tmax)) continue;       // every primitive lies beyond the best hit
            const int key = S.skey[slot], kind = key & 1;
            const float *rec = S.rec + (size_t)slot * S.stride;
            for (int gi = 0; gi < G.n; ++gi) {
                const int bo = G.body[gi];
                RPrim p;
                const Q4 q = *(const float4 *)(rec + 4 * bo);
                const V3 bp = r_ld(rec + 4 * S.R.B + 3 * bo);
                const V3 a = r_add(bp, quat_rotate(q, r_ld(G.p0[gi])));
                const V3 bb = G.type[gi] == PARC_GEOM_CAPSULE ? r_add(bp, quat_rotate(q, r_ld(G.p1[gi]))) : a;
                p.a[0] = a.x; p.a[1] = a.y; p.a[2] = a.z; p.b[0] = bb.x; p.b[1] = bb.y; p.b[2] = bb.z;
                p.s[0] = G.size[gi][0]; p.s[1] = G.size[gi][1]; p.s[2] = G.size[gi][2];
                p.q[0] = q.x; p.q[1] = q.y; p.q[2] = q.z; p.q[3] = q.w;
                p.type = G.type[gi];
                float t;
                V3 nl = mk3(0.f, 0.f, 0.f);
                if (p.type == PARC_GEOM_SPHERE) t = sphere_t(O, d, a, p.s[0]);
                else if (p.type == PARC_GEOM_CAPSULE) t = capsule_t(O, d, a, bb, p.s[0]);
                else t = box_t(O, d, p, nl);
                if (!(t < tmax)) continue;
                // (t, env, kind, geom) in lexicographic order; geoms of one character come in order, so equal t keeps the first
                if (!(t < h.t || (t == h.t && key < sh.key))) continue;
                h.t = t; h.id = (kind == 0 ? 16 : 32) + bo; h.prim = gi;
                sh.key = key; sh.slot = slot;
                const V3 x = r_add(O, r_mul(d, t));
                if (p.type == PARC_GEOM_SPHERE) h.n = r_mul(r_sub(x, a), 1.f / p.s[0]);
                else if (p.type == PARC_GEOM_CAPSULE) {
                    const V3 ba = r_sub(bb, a);
                    const float baba = r_dot(ba, ba);
                    const float u = baba > 0.f ? fminf(fmaxf(r_dot(r_sub(x, a), ba) / baba, 0.f), 1.f) : 0.f;
                    h.n = r_mul(r_sub(r_sub(x, a), r_mul(ba, u)), 1.f / p.s[0]);
                } else h.n = quat_rotate(q, nl);
                hit = true;
                if (ANY) return true;
            }
        }
        const float tnx = d.x != 0.f ? (g.x0 + (float)(i + (sx > 0)) * g.s - O.x) * ix : inf;
        const float tny = d.y != 0.f ? (g.y0 + (float)(j + (sy > 0)) * g.s - O.y) * iy : inf;
        const float tb = fminf(tnx, tny);
        // the next bin starts beyond the best hit (with a margin for the rounding of the crossings) or beyond the ray's end
        if (tb >= t1 || tb > h.t * 1.0001f + 1e-4f) break;
        if (tnx < tny) i += sx; else j += sy;
        if (i < 0 || i >= g.nx || j < 0 || j >= g.ny) break;
    }
    return hit;
}

__global__ __launch_bounds__(256) void k_render_scene(const SceneArgs S) {
    __shared__ RenderGeoms s_geom;
    const int tid = threadIdx.x;
    {
        const int *src = (const int *)S.R.geoms;
        int *dst = (int *)&s_geom;
        for (int w = tid; w < (int)(sizeof(RenderGeoms) / 4); w += 256) dst[w] = src[w];
    }
    __syncthreads();
    const RenderArgs &A = S.R;
    const int px = blockIdx.x * RENDER_TILE + (tid & (RENDER_TILE - 1)), py = blockIdx.y * RENDER_TILE + (tid / RENDER_TILE);
    if (px >= A.W || py >= A.H) return;
    const SceneFrame F = scene_frame(A, S.cam_env);
    const V3 o = r_add(F.t_loc, F.eoc);
    const float gx0 = (A.min_x - o.x) - 0.5f * A.dx, gy0 = (A.min_y - o.y) - 0.5f * A.dy;
    RenderArgs Ar = A;
    Ar.hmax = A.hmax - o.z; Ar.hz = o.z;
    const SceneGrid g = scene_grid(S.hdr);

    const V3 eye = F.eye;
    const float sx = (((float)px + 0.5f) / (float)A.W * 2.f - 1.f) * A.tan_half * A.aspect;
    const float sy = (1.f - ((float)py + 0.5f) / (float)A.H * 2.f) * A.tan_half;
    const V3 d = normalize3(r_add(F.f, r_add(r_mul(F.rt, sx), r_mul(F.up, sy))));

    RHit h;
    h.t = RENDER_NO_HIT; h.id = 0; h.prim = 0; h.n = mk3(0.f, 0.f, 1.f);
    SHit sh; sh.key = 0x7fffffff; sh.slot = -1;
    {
        RHit th;
        if (terrain_hit<false>(Ar, gx0, gy0, eye, d, RENDER_NO_HIT, th)) h = th;
    }
    scene_chars<false>(S, s_geom, g, eye, d, h.t, h, sh);
    const size_t pix = (size_t)py * A.W + px;
    float col[3] = {0.62f, 0.75f, 0.92f}; // sky
    int id = 0;
    if (h.t < RENDER_NO_HIT) {
        id = h.id;
        const V3 sun = r_ld(A.sun);
        V3 n = h.n;
        if (r_dot(n, d) > 0.f) n = r_mul(n, -1.f);
        bool lit = true;
        if (A.shadows) {
            const V3 x = r_add(r_add(eye, r_mul(d, h.t)), r_mul(n, 2e-3f));
            RHit th;
            lit = !terrain_hit<true>(Ar, gx0, gy0, x, sun, RENDER_NO_HIT, th);
            if (lit) {
                RHit ch; ch.t = RENDER_NO_HIT; ch.id = 0; ch.prim = 0; ch.n = mk3(0.f, 0.f, 1.f);
                SHit cs; cs.key = 0x7fffffff; cs.slot = -1;
                lit = !scene_chars<true>(S, s_geom, g, x, sun, RENDER_NO_HIT, ch, cs);
            }
            if (!lit) id |= 0x80;
        }
        float alb[3];
        if (h.id == 1) { const float c = h.prim ? 0.52f : 0.64f; alb[0] = c; alb[1] = c; alb[2] = c; }
        else if (h.id == 2) { alb[0] = 0.42f; alb[1] = 0.42f; alb[2] = 0.46f; }
        else {
            // the colours of k_render; debug_visuals tints the camera env only (ig_parkour_env.py:1046-1064 tints _camera_env_id)
            const int e = sh.key >> 1, b = h.id & 15;
            const bool dbg = A.debug && e == S.cam_env;
            if ((sh.key & 1) == 0) {
                if (dbg) {
                    const float *cf = A.contact_forces + 3 * ((size_t)e * A.B + b);
                    const float f = fminf(fmaxf(sqrtf(cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2]), 0.f), 1.f);
                    alb[0] = 1.f; alb[1] = 1.f - f; alb[2] = 1.f - f;
                } else { alb[0] = 0.45f; alb[1] = 0.6f; alb[2] = 0.95f; }
            } else if (dbg) {
                const float cv = fminf(fmaxf(A.ref_contacts[(size_t)e * A.B + b], 0.f), 1.f);
                alb[0] = cv; alb[1] = 1.f - cv; alb[2] = 0.f;
            } else { alb[0] = 0.5f; alb[1] = 0.9f; alb[2] = 0.1f; }
        }
        const float lam = lit ? fmaxf(r_dot(n, sun), 0.f) : 0.f;
        const float s = 0.35f + 0.65f * lam;
        col[0] = alb[0] * s; col[1] = alb[1] * s; col[2] = alb[2] * s;
    }
    if (A.rgba) {
        uchar4 c;
        c.x = (unsigned char)fminf(col[0] * 255.f + 0.5f, 255.f); c.y = (unsigned char)fminf(col[1] * 255.f + 0.5f, 255.f);
        c.z = (unsigned char)fminf(col[2] * 255.f + 0.5f, 255.f); c.w = 255;
        *(uchar4 *)(A.rgba + 4 * pix) = c;
    }
    if (A.depth) A.depth[pix] = h.t < RENDER_NO_HIT ? h.t : __int_as_float(0x7f800000);
    if (A.id) A.id[pix] = (unsigned char)id;
    if (S.env_map) S.env_map[pix] = sh.slot >= 0 && h.id >= 16 ? sh.key >> 1 : -1;
}
