// parc_render.hpp — headless ray-cast renderer of the env scene (parc_env_render; the reference's viewer, ig_parkour_env.py:417-441,
// :1046-1064, :1123-1132, drawn without a display).  It reuses the FK helpers of the env's operators (joint_dof_to_rot,
// fk_thread); nothing of the step path calls into this file.
//
// Scene = exactly what the physics collides with:
//   terrain    the heightfield as blocky cell columns (terrain_util.py:1099-1184, convert_heightfield_to_voxelized_trimesh): cell (i, j)
//              is solid below hf[i][j] over min + (i, j) dx +- dx/2 (the cell convention of cell_of / sphere_vs_column in
//              parc_dynamics.hpp); vertical walls between neighbours of different height and on the grid's rim; nothing outside the
//              grid.  Traversal is a 2-D DDA (Amanatides & Woo 1987) over the columns, so every step edge is where the contacts see it.
//   characters the MJCF collision geoms (spheres, capsules, boxes) at FK of the simulated state (char_root_pos / rot + char_dof_pos)
//              and, optionally, of the reference mirrors (ref_root_pos / rot + ref_joint_rot, shifted by ref_char_offset).
// World placement is the ray observation's (state + env_offsets).  All intersection arithmetic happens in a frame centred on the camera
// target: the large coordinates (env origin, grid origin) are subtracted once per block, so an env 1 km out renders like one at 0.
//
// Camera (pixel (x, y), y down):  f = normalize(target - eye), r = normalize(f x z) (f x y when f is vertical), u = r x f,
//   dir = normalize(f + sx r + sy u),  sx = ((x + 0.5) / W * 2 - 1) tan(fov_y / 2) W / H,  sy = (1 - (y + 0.5) / H * 2) tan(fov_y / 2).
//
// Kernel shape: one 256-thread block per 16 x 16 pixel tile of one env, grid = (tiles_x, tiles_y, k).  Wave 0 of the block forms the
// joint rotations and FK of both characters and the camera-relative primitives + one bounding sphere per character in LDS (~3 KB); then
// every thread casts its pixel's primary ray and (shadows on) one shadow ray toward the sun with the same intersection code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/parc_env.h"
#include "parc_env_ops.hpp"      // fk_thread
#include "parc_env_tables.hpp"   // DevTables, joint_dof_to_rot
#include "parc_math.hpp"

#define RENDER_MAX_PRIMS (2 * PARC_MAX_GEOMS)
#define RENDER_TILE 16

struct RenderGeoms { // the collision geoms of ParcDynamicsParams, uploaded once at env creation
    int n;
    int body[PARC_MAX_GEOMS];
    int type[PARC_MAX_GEOMS];
    float p0[PARC_MAX_GEOMS][3], p1[PARC_MAX_GEOMS][3], size[PARC_MAX_GEOMS][3];
};

struct RenderArgs {
    int W, H, N, B;
    int cam_mode, draw_ref, shadows, debug;
    float off[3], eye[3], tgt[3], ref_off[3];
    float tan_half, aspect;
    float sun[3];
    const int64_t *env_ids;
    const float *root_pos, *root_rot, *dof_pos, *contact_forces;
    const float *ref_root_pos, *ref_root_rot, *ref_joint_rot, *ref_contacts;
    const float *env_off;
    const float *hf; int X, Y, D; float min_x, min_y, dx, dy, hmax, hz; // hmax: highest column top; hz: height subtracted from every top (the frame's origin)
    const DevTables *tables;
    const RenderGeoms *geoms;
    unsigned char *rgba; float *depth; unsigned char *id;
};

struct RPrim {          // one primitive in the camera-target frame
    float a[3], b[3];   // sphere / box centre | capsule ends
    float s[3];         // sphere r | box half extents | capsule r
    float q[4];         // box orientation (x, y, z, w)
    float col[3];
    float bound;        // distance of the farthest point from the character's root
    int type, id;
};

struct RHit {
    float t;
    V3 n;
    int id;     // 0 sky, 1 terrain top, 2 terrain wall, 16 + b / 32 + b bodies
    int prim;   // character primitive, or the checker parity of a top face
};

#define RENDER_NO_HIT 3.0e38f

__device__ __forceinline__ V3 r_add(V3 a, V3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 r_sub(V3 a, V3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 r_mul(V3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float r_dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 r_ld(const float *p) { return mk3(p[0], p[1], p[2]); }

// ---- terrain: 2-D DDA over the columns ------------------------------------------------------------------------------------------------
// gx0 / gy0: low edge of cell 0 in the camera-target frame (A.hmax / A.hz already moved into it).  Returns the nearest top / wall hit with t in [0, tmax).
template <bool ANY>
__device__ __forceinline__ bool terrain_hit(const RenderArgs &A, float gx0, float gy0, V3 O, V3 d, float tmax, RHit &h) {
    const float inf = RENDER_NO_HIT;
    const float ix = d.x != 0.f ? 1.f / d.x : inf, iy = d.y != 0.f ? 1.f / d.y : inf;
    const float gx1 = gx0 + (float)A.X * A.dx, gy1 = gy0 + (float)A.Y * A.dy;
    float t0 = 0.f, t1 = tmax;
    int axis = -1; // axis of the face the ray enters the grid through (-1: starts inside)
    if (d.x != 0.f) {
        const float ta = (gx0 - O.x) * ix, tb = (gx1 - O.x) * ix;
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        if (lo > t0) { t0 = lo; axis = 0; }
        t1 = fminf(t1, hi);
    } else if (O.x < gx0 || O.x >= gx1) return false;
    if (d.y != 0.f) {
        const float ta = (gy0 - O.y) * iy, tb = (gy1 - O.y) * iy;
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        if (lo > t0) { t0 = lo; axis = 1; }
        t1 = fminf(t1, hi);
    } else if (O.y < gy0 || O.y >= gy1) return false;
    // no column reaches above hmax: the part of the ray above it cannot hit
    if (d.z < 0.f) { const float tz = (A.hmax - O.z) / d.z; if (tz > t0) { t0 = tz; axis = 2; } }
    else if (O.z >= A.hmax) return false;
    else if (d.z > 0.f) t1 = fminf(t1, (A.hmax - O.z) / d.z);
    if (!(t0 < t1)) return false;
    const V3 P = r_add(O, r_mul(d, t0));
    int i = (int)floorf((P.x - gx0) / A.dx), j = (int)floorf((P.y - gy0) / A.dy);
    i = min(max(i, 0), A.X - 1); j = min(max(j, 0), A.Y - 1);
    const int sx = d.x > 0.f ? 1 : -1, sy = d.y > 0.f ? 1 : -1;
    float ta = t0;
    const int max_steps = A.X + A.Y + 2;
    for (int it = 0; it < max_steps; ++it) {
        const float top = A.hf[(size_t)i * A.Y + j] - A.hz;
        const float tnx = d.x != 0.f ? (gx0 + (float)(i + (sx > 0)) * A.dx - O.x) * ix : inf;
        const float tny = d.y != 0.f ? (gy0 + (float)(j + (sy > 0)) * A.dy - O.y) * iy : inf;
        const float tb = fminf(fminf(tnx, tny), t1);
        const float za = O.z + d.z * ta;
        if (za < top && axis != 2) { // entered this column below its top: a wall (or the camera sits inside a column)
            h.t = ta; h.id = 2; h.prim = 0;
            h.n = axis == 0 ? mk3((float)-sx, 0.f, 0.f) : (axis == 1 ? mk3(0.f, (float)-sy, 0.f) : r_mul(d, -1.f));
            return true;
        }
        if (d.z < 0.f) {
            const float th = (top - O.z) / d.z;
            if (th <= tb) {
                h.t = fmaxf(th, ta); h.id = 1; h.prim = (i + j) & 1; h.n = mk3(0.f, 0.f, 1.f);
                return true;
            }
        }
        if (tb >= t1) return false;
        if (tnx < tny) { i += sx; ta = tnx; axis = 0; } else { j += sy; ta = tny; axis = 1; }
        if (i < 0 || i >= A.X || j < 0 || j >= A.Y) return false;
    }
    return false;
}

// ---- character primitives --------------------------------------------------------------------------------------------------------------
#define RENDER_TMIN 1e-4f

__device__ __forceinline__ float sphere_t(V3 O, V3 d, V3 c, float r) {
    const V3 oc = r_sub(O, c);
    const float b = r_dot(oc, d), cc = r_dot(oc, oc) - r * r, disc = b * b - cc;
    if (disc < 0.f) return RENDER_NO_HIT;
    const float t = -b - sqrtf(disc);
    return t > RENDER_TMIN ? t : RENDER_NO_HIT;
}

__device__ __forceinline__ float capsule_t(V3 O, V3 d, V3 a, V3 b, float r) {
    const V3 ba = r_sub(b, a), oa = r_sub(O, a);
    const float baba = r_dot(ba, ba), bard = r_dot(ba, d), baoa = r_dot(ba, oa), rdoa = r_dot(d, oa), oaoa = r_dot(oa, oa);
    const float qa = baba - bard * bard, qb = baba * rdoa - baoa * bard, qc = baba * oaoa - baoa * baoa - r * r * baba;
    const float hh = qb * qb - qa * qc;
    if (hh >= 0.f && qa > 1e-12f) {
        const float t = (-qb - sqrtf(hh)) / qa, y = baoa + t * bard;
        if (y > 0.f && y < baba) return t > RENDER_TMIN ? t : RENDER_NO_HIT;
    }
    // the end caps: the nearer of the two spheres
    return fminf(sphere_t(O, d, a, r), sphere_t(O, d, b, r));
}

__device__ __forceinline__ float box_t(V3 O, V3 d, const RPrim &p, V3 &nl) {
    const Q4 qi = mk4(-p.q[0], -p.q[1], -p.q[2], p.q[3]);
    const V3 o = quat_rotate(qi, r_sub(O, r_ld(p.a))), dl = quat_rotate(qi, d);
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {dl.x, dl.y, dl.z};
    float tn = -RENDER_NO_HIT, tf = RENDER_NO_HIT;
    int ax = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dd[k] == 0.f) {
            if (fabsf(oo[k]) > p.s[k]) return RENDER_NO_HIT;
            continue;
        }
        const float inv = 1.f / dd[k];
        const float t1 = (-p.s[k] - oo[k]) * inv, t2 = (p.s[k] - oo[k]) * inv;
        const float lo = fminf(t1, t2), hi = fmaxf(t1, t2);
        if (lo > tn) { tn = lo; ax = k; }
        tf = fminf(tf, hi);
    }
    if (!(tn <= tf) || !(tn > RENDER_TMIN)) return RENDER_NO_HIT;
    nl = mk3(ax == 0 ? (dd[0] > 0.f ? -1.f : 1.f) : 0.f, ax == 1 ? (dd[1] > 0.f ? -1.f : 1.f) : 0.f, ax == 2 ? (dd[2] > 0.f ? -1.f : 1.f) : 0.f);
    return tn;
}

// Nearest primitive of the characters (bounding sphere first); ANY: stop at the first hit (shadow rays).
template <bool ANY>
__device__ __forceinline__ bool chars_hit(const RPrim *prims, const float *bsph, int nchar, int ng, V3 O, V3 d, float tmax, RHit &h) {
    bool hit = false;
    for (int c = 0; c < nchar; ++c) {
        const V3 bc = mk3(bsph[4 * c], bsph[4 * c + 1], bsph[4 * c + 2]);
        const V3 oc = r_sub(O, bc);
        const float b = r_dot(oc, d), cc = r_dot(oc, oc) - bsph[4 * c + 3] * bsph[4 * c + 3];
        if (b * b - cc < 0.f || (b > 0.f && cc > 0.f)) continue; // misses, or points away from a sphere the origin is outside of
        for (int g = 0; g < ng; ++g) {
            const RPrim &p = prims[c * PARC_MAX_GEOMS + g];
            float t;
            V3 nl = mk3(0.f, 0.f, 0.f);
            if (p.type == PARC_GEOM_SPHERE) t = sphere_t(O, d, r_ld(p.a), p.s[0]);
            else if (p.type == PARC_GEOM_CAPSULE) t = capsule_t(O, d, r_ld(p.a), r_ld(p.b), p.s[0]);
            else t = box_t(O, d, p, nl);
            if (t < tmax && t < h.t) {
                h.t = t; h.id = p.id; h.prim = c * PARC_MAX_GEOMS + g;
                const V3 x = r_add(O, r_mul(d, t));
                if (p.type == PARC_GEOM_SPHERE) h.n = r_mul(r_sub(x, r_ld(p.a)), 1.f / p.s[0]);
                else if (p.type == PARC_GEOM_CAPSULE) {
                    const V3 a = r_ld(p.a), ba = r_sub(r_ld(p.b), a);
                    const float baba = r_dot(ba, ba);
                    const float u = baba > 0.f ? fminf(fmaxf(r_dot(r_sub(x, a), ba) / baba, 0.f), 1.f) : 0.f;
                    h.n = r_mul(r_sub(r_sub(x, a), r_mul(ba, u)), 1.f / p.s[0]);
                } else h.n = quat_rotate(mk4(p.q[0], p.q[1], p.q[2], p.q[3]), nl);
                hit = true;
                if (ANY) return true;
            }
        }
    }
    return hit;
}

template <bool ANY>
__device__ __forceinline__ bool scene_hit(const RenderArgs &A, const RPrim *prims, const float *bsph, int nchar, int ng, float gx0, float gy0,
                                          V3 O, V3 d, RHit &h) {
    h.t = RENDER_NO_HIT; h.id = 0; h.prim = 0; h.n = mk3(0.f, 0.f, 1.f);
    RHit th;
    bool hit = false;
    if (terrain_hit<ANY>(A, gx0, gy0, O, d, RENDER_NO_HIT, th)) {
        h = th; hit = true;
        if (ANY) return true;
    }
    return chars_hit<ANY>(prims, bsph, nchar, ng, O, d, h.t, h) || hit;
}

__global__ __launch_bounds__(256) void k_render(const RenderArgs A) {
    __shared__ float4 s_jr[2][PARC_MAX_BODIES];                    // joint rotations, index j - 1
    __shared__ float s_bp[2][3 * PARC_MAX_BODIES];
    __shared__ float4 s_br[2][PARC_MAX_BODIES];
    __shared__ RPrim s_prim[RENDER_MAX_PRIMS];
    __shared__ float s_bsph[8];                                    // bounding sphere (centre, radius) per character

    const int tid = threadIdx.x;
    const int k = blockIdx.z;
    const int e = A.env_ids ? (int)A.env_ids[k] : k;
    if (e < 0 || e >= A.N) return;                                  // block-uniform (the host validates the ids it can see)
    const int B = A.B, ng = A.geoms->n, nchar = A.draw_ref ? 2 : 1;

    // camera-target frame: t_loc = target in env-local coordinates, o = the same point in world coordinates (formed once)
    const V3 root = r_ld(A.root_pos + 3 * (size_t)e);
    const V3 eo = r_ld(A.env_off + 3 * (size_t)e);
    const V3 t_loc = A.cam_mode == 0 ? root : r_ld(A.tgt);
    const V3 o = r_add(t_loc, eo);
    const float gx0 = (A.min_x - o.x) - 0.5f * A.dx, gy0 = (A.min_y - o.y) - 0.5f * A.dy;
    RenderArgs Ar = A;                                              // heights relative to the target as well
    Ar.hmax = A.hmax - o.z; Ar.hz = o.z;

    // ---- prologue (wave 0): joint rotations, FK, primitives, bounding spheres ----
    if (tid < 64) {
        const int c = tid >> 5, j = tid & 31;
        if (j >= 1 && j < B) {
            if (c == 0) {
                s_jr[0][j - 1] = joint_dof_to_rot(A.tables->h.jtype[j], A.tables->h.axis[j], A.dof_pos + (size_t)A.D * e + A.tables->h.dof_idx[j]);
            } else if (A.draw_ref) {
                s_jr[1][j - 1] = *(const float4 *)(A.ref_joint_rot + 4 * ((size_t)e * (B - 1) + j - 1));
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float *rr = A.root_rot + 4 * (size_t)e;
        fk_thread(A.tables, B, r_sub(root, t_loc), mk4(rr[0], rr[1], rr[2], rr[3]), (const float *)s_jr[0], s_bp[0], (float *)s_br[0]);
    } else if (tid == 32 && A.draw_ref) {
        const float *rp = A.ref_root_pos + 3 * (size_t)e, *rr = A.ref_root_rot + 4 * (size_t)e;
        const V3 p = mk3(rp[0] + A.ref_off[0] - t_loc.x, rp[1] + A.ref_off[1] - t_loc.y, rp[2] + A.ref_off[2] - t_loc.z);
        fk_thread(A.tables, B, p, mk4(rr[0], rr[1], rr[2], rr[3]), (const float *)s_jr[1], s_bp[1], (float *)s_br[1]);
    }
    __syncthreads();
    if (tid < 64) {
        const int c = tid >> 5, g = tid & 31;
        if (g < ng && c < nchar) {
            const RenderGeoms &G = *A.geoms;
            const int b = G.body[g];
            const Q4 q = s_br[c][b];
            const V3 bp = r_ld(&s_bp[c][3 * b]);
            RPrim p;
            const V3 a = r_add(bp, quat_rotate(q, r_ld(G.p0[g])));
            const V3 bb = G.type[g] == PARC_GEOM_CAPSULE ? r_add(bp, quat_rotate(q, r_ld(G.p1[g]))) : a;
            p.a[0] = a.x; p.a[1] = a.y; p.a[2] = a.z; p.b[0] = bb.x; p.b[1] = bb.y; p.b[2] = bb.z;
            p.s[0] = G.size[g][0]; p.s[1] = G.size[g][1]; p.s[2] = G.size[g][2];
            p.q[0] = q.x; p.q[1] = q.y; p.q[2] = q.z; p.q[3] = q.w;
            p.type = G.type[g];
            p.id = (c == 0 ? 16 : 32) + b;
            const V3 r0 = r_ld(&s_bp[c][0]);
            const float ext = G.type[g] == PARC_GEOM_BOX ? sqrtf(p.s[0] * p.s[0] + p.s[1] * p.s[1] + p.s[2] * p.s[2]) : p.s[0];
            p.bound = fmaxf(norm3(r_sub(a, r0)), norm3(r_sub(bb, r0))) + ext;
            // colours: simulated character light blue, reference (0.5, 0.9, 0.1) (ig_parkour_env.py:418).  debug_visuals
            // (ig_parkour_env.py:1046-1064): simulated bodies white -> red by |contact force| and reference bodies green -> red by the target
            // contact.  Deviation: the force factor is clamped to [0, 1]; the reference extrapolates past 1 (a colour component < 0).
            if (c == 0) {
                float f = 0.f;
                if (A.debug) {
                    const float *cf = A.contact_forces + 3 * ((size_t)e * B + b);
                    f = fminf(fmaxf(sqrtf(cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2]), 0.f), 1.f);
                    p.col[0] = 1.f; p.col[1] = 1.f - f; p.col[2] = 1.f - f;
                } else { p.col[0] = 0.45f; p.col[1] = 0.6f; p.col[2] = 0.95f; }
            } else if (A.debug) {
                const float cv = fminf(fmaxf(A.ref_contacts[(size_t)e * B + b], 0.f), 1.f);
                p.col[0] = cv; p.col[1] = 1.f - cv; p.col[2] = 0.f;
            } else { p.col[0] = 0.5f; p.col[1] = 0.9f; p.col[2] = 0.1f; }
            s_prim[c * PARC_MAX_GEOMS + g] = p;
        }
    }
    __syncthreads();
    if (tid < 2) {
        float r = 0.f;
        if (tid < nchar)
            for (int g = 0; g < ng; ++g) r = fmaxf(r, s_prim[tid * PARC_MAX_GEOMS + g].bound);
        s_bsph[4 * tid] = s_bp[tid][0]; s_bsph[4 * tid + 1] = s_bp[tid][1]; s_bsph[4 * tid + 2] = s_bp[tid][2];
        s_bsph[4 * tid + 3] = r * 1.0001f + 1e-4f;
    }
    __syncthreads();

    // ---- one primary ray per thread ----
    const int px = blockIdx.x * RENDER_TILE + (tid & (RENDER_TILE - 1)), py = blockIdx.y * RENDER_TILE + (tid / RENDER_TILE);
    if (px >= A.W || py >= A.H) return;
    const V3 eye = A.cam_mode == 0 ? r_ld(A.off) : r_sub(r_ld(A.eye), t_loc);
    const V3 f = normalize3(r_mul(eye, -1.f));
    V3 rt = cross3(f, mk3(0.f, 0.f, 1.f));
    if (norm3(rt) < 1e-6f) rt = cross3(f, mk3(0.f, 1.f, 0.f));
    rt = normalize3(rt);
    const V3 up = cross3(rt, f);
    const float sx = (((float)px + 0.5f) / (float)A.W * 2.f - 1.f) * A.tan_half * A.aspect;
    const float sy = (1.f - ((float)py + 0.5f) / (float)A.H * 2.f) * A.tan_half;
    const V3 d = normalize3(r_add(f, r_add(r_mul(rt, sx), r_mul(up, sy))));

    RHit h;
    scene_hit<false>(Ar, s_prim, s_bsph, nchar, ng, gx0, gy0, eye, d, h);
    const size_t pix = ((size_t)k * A.H + py) * A.W + px;
    float col[3] = {0.62f, 0.75f, 0.92f}; // sky
    int id = 0;
    if (h.t < RENDER_NO_HIT) {
        id = h.id;
        const V3 sun = r_ld(A.sun);
        V3 n = h.n;
        if (r_dot(n, d) > 0.f) n = r_mul(n, -1.f); // two-sided (a camera inside a column)
        bool lit = true;
        if (A.shadows) {
            const V3 x = r_add(r_add(eye, r_mul(d, h.t)), r_mul(n, 2e-3f));
            RHit sh;
            lit = !scene_hit<true>(Ar, s_prim, s_bsph, nchar, ng, gx0, gy0, x, sun, sh);
            if (!lit) id |= 0x80;
        }
        float alb[3];
        if (h.id == 1) { const float c = h.prim ? 0.52f : 0.64f; alb[0] = c; alb[1] = c; alb[2] = c; }      // checker by cell parity
        else if (h.id == 2) { alb[0] = 0.42f; alb[1] = 0.42f; alb[2] = 0.46f; }
        else { const RPrim &p = s_prim[h.prim]; alb[0] = p.col[0]; alb[1] = p.col[1]; alb[2] = p.col[2]; }
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
}
