// parc_mpath_select.hpp — rollout selection on gfx950 (parc_msel_*, include/parc_env.h): the scoring step of
// mdm_path.generate_frames_until_end_of_path (mdm_path.py:386-433) and the acceptance test of parc_2_kin_gen.py:389-404 for the N rows of
// a rollout, on the device buffers parc_mpath_rollout left.  With slice_terrain every row is scored on its own slice of its terrain
// (terrain_util.slice_terrain_around_motion, padding 1.2, localize=False), which is never materialised for the scoring: the slice is two
// small index tables into the parent terrain.
//   k_msel_bounds   a wave per row: n = len(frames[0:final_frame]); the root's xy bounds, the slice's grid points (torch.arange's count and
//                   values), the parent index of every slice column / row, the lowest height of the view, the status bits
//   k_msel_fk       a lane per (row, frame < n): validity of the inputs, FK (fk_frame) into the workspace
//   k_msel_score    a block per (row, frame < n), a lane per sample point: compute_motion_loss against the row's view (the analyser's
//                   terrain_sdf through the index tables), per body the penetration sum and the contact term, lane 0 the frame's two sums
//   k_msel_rank     a wave per path: per row the frames in order (double accumulator), the weights, the penalty, the noise, the
//                   thresholds; the stable ascending order of the path's rows, NaN last; the count of valid rows
//   k_msel_gather   a block per named row: its sliced heightfield to its place in the packed output (offsets from the host's scan)
// No float atomics and no reduction whose order depends on the batch: a row's results are the same bits alone or in any batch.
#pragma once
#include "parc_mdm_path.hpp"
#include "parc_motion_terrain.hpp"
#include "parc_tool_handle.hpp"

namespace msel {
using namespace parc;

constexpr int WV = 64;
constexpr int SC_THREADS = 256;
constexpr int MAXD = PARC_MSEL_MAX_SLICE_DIM;
constexpr int MAXP = PARC_MOPT_MAX_POINTS;
constexpr int MAXB = PARC_MAX_BODIES;

struct View {                              // a row's terrain as the scoring sees it (k_msel_bounds writes it)
    int n, status, sx, sy;                 // frames scored; PARC_MSEL_STATUS_*; the view's dims
    float mnx, mny, base_z;                // its min point; min height - 10 (compute_motion_loss)
    int sliced;                            // heights through the row's index tables, else the terrain's own array
};
struct Cfg {                               // by value
    float w_contact, w_pen, penalty, padding;
    int sdf_mode;
};
struct Work {
    View *view;                            // [N]
    int *ix, *iy;                          // [N][MAXD]: the parent index of every slice column / row
    float *pos, *rot;                      // [N][max_frames][B][3], [..][4]
    int *valid;                            // [N][max_frames] inputs finite
    float *fterms;                         // [N][max_frames][2]: pen, contact
    float *contact, *pen, *total;          // [N]
    int *ok, *order, *num_valid;           // [N] valid, [N] rows grouped by path and sorted, [P]
    int max_frames;
};
struct Frames {                            // the caller's buffers
    const float *frames;                   // [N][stride][FD]
    const int *final_frame;                // [N]
    const float *noise;                    // [N] or null
    int num_frames, stride;
};

// a slice of the parent terrain: cell (a, b) is parent cell (ix[a], iy[b])
struct HfRowIndexed {
    const float *row;
    const int *iy;
    __device__ __forceinline__ float operator[](long long j) const { return row[iy[j]]; }
};
struct HfIndexed {
    const float *hf;
    const int *ix, *iy;
    long long Yp;
    __device__ __forceinline__ HfRowIndexed row(long long i) const { return HfRowIndexed{hf + (long long)ix[i] * Yp, iy}; }
};

// round_point_to_grid_point (terrain_util.py:143): fp32, a true division
__device__ __forceinline__ float grid_point(float p, float mn, float d) { return rintf((p - mn) / d) * d + mn; }
// torch.arange(start, end, step) of fp32 scalars: the size in double
__device__ __forceinline__ double arange_count(float start, float end, float step) { return ceil(((double)end - (double)start) / (double)step); }
__device__ __forceinline__ float arange_at(float start, float step, int i) { return (float)((double)start + (double)step * (double)i); }

__device__ __forceinline__ float wave_min(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, WV));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WV));
    return v;
}

__global__ void __launch_bounds__(WV) k_msel_bounds(mpath::Scene S, Frames R, Cfg G, int FD, int slice_terrain, Work W) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int p = S.row_path[row], ff = R.final_frame[row];
    int n = ff < 0 ? R.num_frames + ff : min(ff, R.num_frames);   // frames[0:final_frame] as Python slices it
    n = max(n, 0);
    const float *hf = S.hf + (size_t)p * S.X * S.Y;
    const float minx = S.minp[2 * p], miny = S.minp[2 * p + 1];
    int *ix = W.ix + (size_t)row * MAXD, *iy = W.iy + (size_t)row * MAXD;
    View v;
    v.n = n; v.status = n < 1 ? PARC_MSEL_STATUS_EMPTY : 0;
    v.sx = S.X; v.sy = S.Y; v.mnx = minx; v.mny = miny; v.sliced = 0;
    float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
    int bad = 0;
    for (int f = lane; f < n; f += WV) {
        const float *src = R.frames + ((size_t)row * R.stride + f) * FD;
        const float x = src[0], y = src[1], z = src[2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) bad = 1;
        lo_x = fminf(lo_x, x); hi_x = fmaxf(hi_x, x);
        lo_y = fminf(lo_y, y); hi_y = fmaxf(hi_y, y);
    }
    if (__any(bad)) v.status |= PARC_MSEL_STATUS_NONFINITE;
    float hmin = INFINITY;
    if (slice_terrain && v.status == 0) {
        lo_x = wave_min(lo_x); lo_y = wave_min(lo_y); hi_x = wave_max(hi_x); hi_y = wave_max(hi_y);
        const float g0x = grid_point(lo_x - G.padding, minx, S.dx), g0y = grid_point(lo_y - G.padding, miny, S.dy);
        const float g1x = grid_point(hi_x + G.padding, minx, S.dx), g1y = grid_point(hi_y + G.padding, miny, S.dy);
        const double cx = arange_count(g0x, g1x + S.dx, S.dx), cy = arange_count(g0y, g1y + S.dy, S.dy);
        if (!(cx >= 1.0 && cx <= (double)MAXD && cy >= 1.0 && cy <= (double)MAXD)) {
            v.status |= PARC_MSEL_STATUS_TOO_LARGE;
        } else {
            v.sx = (int)cx; v.sy = (int)cy; v.mnx = g0x; v.mny = g0y; v.sliced = 1;
            for (int a = lane; a < v.sx; a += WV) ix[a] = (int)grid_index(arange_at(g0x, S.dx, a), minx, S.dx, S.X);
            for (int b = lane; b < v.sy; b += WV) iy[b] = (int)grid_index(arange_at(g0y, S.dy, b), miny, S.dy, S.Y);
            __syncthreads();               // one wave: the tables written above are read below
            const HfIndexed H{hf, ix, iy, S.Y};
            const int cells = v.sx * v.sy;
            for (int c = lane; c < cells; c += WV) hmin = fminf(hmin, H.row(c / v.sy)[c % v.sy]);
        }
    } else if (v.status == 0) {
        const long long cells = (long long)S.X * S.Y;
        for (long long c = lane; c < cells; c += WV) hmin = fminf(hmin, hf[c]);
    }
    hmin = wave_min(hmin);
    v.base_z = (float)((double)hmin - 10.0);
    if (lane == 0) W.view[row] = v;
}

__global__ void k_msel_fk(const CharPoints *Mp, Frames R, int N, int FD, Work W) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * R.num_frames) return;
    const int row = (int)(i / R.num_frames), f = (int)(i - (long long)row * R.num_frames);
    const View &v = W.view[row];
    if (v.status || f >= v.n) return;
    const CharPoints &M = *Mp;
    const int B = M.B;
    const float *src = R.frames + ((size_t)row * R.stride + f) * FD;
    const long long w = (long long)row * W.max_frames + f;
    bool ok = true;
    for (int k = 0; k < FD; ++k) ok = ok && isfinite(src[k]);
    // fk_frame reads joint j's rotation at base + 4 j for j >= 1 only: joint j's is at src + 7 + 4 (j - 1)
    fk_frame(M, ld3(src), ld4(src + 3), src + 3, W.pos + w * B * 3, W.rot + w * B * 4);
    W.valid[w] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(SC_THREADS) k_msel_score(const CharPoints *Mp, mpath::Scene S, Frames R, Cfg G, int FD, Work W) {
    __shared__ float s_c[MAXP], s_pen[MAXP];
    __shared__ float s_body[MAXB][2];
    __shared__ int s_bad;
    const int row = blockIdx.x / R.num_frames, f = blockIdx.x - row * R.num_frames, tid = threadIdx.x;
    const View v = W.view[row];
    if (v.status || f >= v.n) return;
    const CharPoints &M = *Mp;
    const int B = M.B, P = M.P, p = S.row_path[row];
    const long long w = (long long)row * W.max_frames + f;
    const float *pos = W.pos + w * B * 3, *rot = W.rot + w * B * 4;
    const float *hf = S.hf + (size_t)p * S.X * S.Y;
    const float *contacts = R.frames + ((size_t)row * R.stride + f) * FD + 7 + 4 * (B - 1);
    if (tid == 0) s_bad = W.valid[w] ? 0 : 1;
    __syncthreads();
    for (int k = tid; k < P; k += SC_THREADS) {
        const int b = M.pt_body[k];
        const V3 x = add3(quat_rotate(ld4(rot + 4 * b), mk3(M.pts[k][0], M.pts[k][1], M.pts[k][2])), ld3(pos + 3 * b));
        float sg = 0.f, sa = 0.f;
        if (!mterr::fin3(x)) s_bad = 1;
        else if (v.sliced)
            mterr::terrain_sdf(x, HfIndexed{hf, W.ix + (size_t)row * MAXD, W.iy + (size_t)row * MAXD, S.Y}, v.sx, v.sy, v.mnx, v.mny, S.dx, S.dy, v.base_z,
                               G.sdf_mode, sg, sa);
        else
            mterr::terrain_sdf(x, hf, v.sx, v.sy, v.mnx, v.mny, S.dx, S.dy, v.base_z, G.sdf_mode, sg, sa);
        s_c[k] = fmaxf(sg, 0.f);           // clamp(positive_sdfs, min=0)
        s_pen[k] = fmaxf(sa, 0.f);         // -clamp(-air, max=0)
    }
    __syncthreads();
    if (tid < B) {                         // per body: the penetration sum in point order, the contact term
        const int b = tid, k0 = M.pt_start[b], np = M.pt_count[b];
        float pen = 0.f, best = INFINITY;
        for (int k = k0; k < k0 + np; ++k) { pen += s_pen[k]; best = fminf(best, s_c[k]); }
        const int cid = M.contact_id[b];
        s_body[b][0] = pen;
        s_body[b][1] = (cid >= 0 && np > 0) ? best * contacts[cid] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float t0 = 0.f, t1 = 0.f;
        for (int b = 0; b < B; ++b) { t0 += s_body[b][0]; t1 += s_body[b][1]; }
        const float nan = __int_as_float(0x7fc00000);
        W.fterms[2 * w] = s_bad ? nan : t0;
        W.fterms[2 * w + 1] = s_bad ? nan : t1;
    }
}

// a sorts before b: ascending, NaN last, the lower row first among equals (torch.sort, stable)
__device__ __forceinline__ bool sorts_before(float a, int i, float b, int j) {
    const bool an = !(a == a), bn = !(b == b);
    if (an || bn) return an == bn ? i < j : bn;
    return a < b || (a == b && i < j);
}

__global__ void __launch_bounds__(WV) k_msel_rank(mpath::Scene S, Frames R, Cfg G, float max_contact, float max_pen, float max_total, Work W) {
    const int p = blockIdx.x, lane = threadIdx.x, N = S.N;
    const float nan = __int_as_float(0x7fc00000);
    int before = 0, nvalid = 0;            // rows of lower paths; this path's valid rows
    for (int r = lane; r < N; r += WV) {
        const int q = S.row_path[r];
        before += q < p ? 1 : 0;
        if (q != p) continue;
        const View &v = W.view[r];
        float contact = nan, pen = nan, total = nan;
        if (!v.status) {
            double sp = 0.0, sc = 0.0;     // the frames in order, as k_mterr_reduce
            const float *t = W.fterms + 2 * (long long)r * W.max_frames;
            for (int f = 0; f < v.n; ++f) { sp += (double)t[2 * f]; sc += (double)t[2 * f + 1]; }
            contact = G.w_contact * (float)sc;
            pen = G.w_pen * (float)sp;
            total = contact + pen;
            if (R.final_frame[r] < 0) total = total + G.penalty;
            if (R.noise) total = total + R.noise[r];
        }
        const int ok = (contact < max_contact && pen < max_pen && total < max_total) ? 1 : 0;
        W.contact[r] = contact; W.pen[r] = pen; W.total[r] = total; W.ok[r] = ok;
        nvalid += ok;
    }
    for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o, WV); nvalid += __shfl_xor(nvalid, o, WV); }
    __syncthreads();                       // one wave: the totals written above are read below
    for (int r = lane; r < N; r += WV) {
        if (S.row_path[r] != p) continue;
        const float t = W.total[r];
        int rank = 0;
        for (int q = 0; q < N; ++q)
            if (S.row_path[q] == p && sorts_before(W.total[q], q, t, r)) ++rank;
        W.order[before + rank] = r;
    }
    if (lane == 0) W.num_valid[p] = nvalid;
}

__global__ void k_msel_gather(mpath::Scene S, Work W, const int *rows, const long long *off, float *out) {
    const int row = rows[blockIdx.x];
    const View &v = W.view[row];
    if (v.status) return;
    const float *hf = S.hf + (size_t)S.row_path[row] * S.X * S.Y;
    const int *ix = W.ix + (size_t)row * MAXD, *iy = W.iy + (size_t)row * MAXD;
    float *o = out + off[blockIdx.x];
    const int cells = v.sx * v.sy;
    for (int c = threadIdx.x; c < cells; c += blockDim.x) {
        const int a = c / v.sy, b = c - a * v.sy;
        o[c] = v.sliced ? hf[(size_t)ix[a] * S.Y + iy[b]] : hf[c];
    }
}
}  // namespace msel

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
// device: the path handle's; ev: 0 .. 4 around the four kernels of a run, 5 .. 6 around k_msel_gather
struct ParcPathSelect : tool::CharHandle<parc::CharPoints, DeviceEvents<7>> {
    ParcMdmPath *mpath = nullptr;
    msel::Cfg cfg{};
    msel::Work W{};
    int max_rows = 0, FD = 0;
    int last_rows = 0, last_P = 0, last_X = 0, last_Y = 0, last_launches = 0;
    bool ran = false, gathered = false;
    std::vector<msel::View> views;         // the host's copy, of the last parc_msel_results / parc_msel_gather
};

extern "C" void parc_msel_destroy(ParcPathSelect *h) { tool::destroy(h); }

extern "C" int parc_msel_create(const ParcPathSelectParams *p, ParcPathSelect **out) {
    PARC_TRY(tool::create_args("msel", "ParcPathSelectParams", p, out));
    if (!p->mpath) return fail(PARC_ERR_INVALID, "msel: mpath is null (the path handle whose rollouts are scored)");
    if (p->num_points < 1 || p->num_points > PARC_MOPT_MAX_POINTS || !p->points_host || !p->point_body_host)
        return fail(PARC_ERR_INVALID, "msel: num_points must be in [1, 512] with points and point bodies given");
    if (p->sdf_mode != PARC_MTERR_SDF_PRUNED && p->sdf_mode != PARC_MTERR_SDF_BRUTE) return fail(PARC_ERR_INVALID, "msel: unknown sdf_mode");
    if (!std::isfinite(p->w_contact) || !std::isfinite(p->w_pen) || !std::isfinite(p->not_finished_penalty))
        return fail(PARC_ERR_INVALID, "msel: w_contact, w_pen and not_finished_penalty must be finite");
    if (!(p->slice_padding >= 0.f) || !std::isfinite(p->slice_padding)) return fail(PARC_ERR_INVALID, "msel: slice_padding must be >= 0");
    ParcMdmPath *g = p->mpath;
    parc::CharPoints M;
    model_zero(M);
    static_cast<parc::CharTree &>(M) = g->mdm->host_model;
    PARC_TRY(model_points("msel", M, p->num_points, p->points_host, p->point_body_host, p->contact_body_id));
    return tool::create("msel", g->device, M, out, [&](ParcPathSelect &h) -> int {
        h.mpath = g; h.max_rows = g->max_batch; h.FD = g->FD;
        h.cfg.w_contact = p->w_contact; h.cfg.w_pen = p->w_pen; h.cfg.penalty = p->not_finished_penalty; h.cfg.padding = p->slice_padding;
        h.cfg.sdf_mode = p->sdf_mode;
        const long long N = h.max_rows, F = g->max_frames, B = M.B;
        msel::Work &W = h.W;
        W.max_frames = g->max_frames;
        PARC_TRY(h.mem.alloc_fill(W.view, N));
        PARC_TRY(h.mem.alloc_fill(W.ix, N * msel::MAXD));
        PARC_TRY(h.mem.alloc_fill(W.iy, N * msel::MAXD));
        PARC_TRY(h.mem.alloc(W.pos, N * F * B * 3));
        PARC_TRY(h.mem.alloc(W.rot, N * F * B * 4));
        PARC_TRY(h.mem.alloc(W.valid, N * F));
        PARC_TRY(h.mem.alloc(W.fterms, N * F * 2));
        PARC_TRY(h.mem.alloc_fill(W.contact, N));
        PARC_TRY(h.mem.alloc_fill(W.pen, N));
        PARC_TRY(h.mem.alloc_fill(W.total, N));
        PARC_TRY(h.mem.alloc_fill(W.ok, N));
        PARC_TRY(h.mem.alloc_fill(W.order, N));
        PARC_TRY(h.mem.alloc_fill(W.num_valid, N));   // a scene has at most as many paths as rows
        return PARC_OK;
    });
}

extern "C" int parc_msel_run(ParcPathSelect *h, const ParcPathSelectArgs *a, void *stream) {
    if (!h || !a) return fail(PARC_ERR_INVALID, "msel: null argument");
    if (!h->mpath->have_scene) return fail(PARC_ERR_STATE, "msel: no scene: parc_mpath_set_scene first");
    if (!a->frames || !a->final_frame) return fail(PARC_ERR_INVALID, "msel: run: frames and final_frame must be given");
    if (a->num_frames < 1 || a->num_frames > a->frame_stride)
        return fail(PARC_ERR_INVALID, "msel: run: num_frames must be 1 .. frame_stride = " + std::to_string(a->frame_stride) + " (the frames a row of the buffer holds)");
    if (a->num_frames > h->W.max_frames)
        return fail(PARC_ERR_INVALID, "msel: run: num_frames exceeds the path handle's max_frames = " + std::to_string(h->W.max_frames));
    if (std::isnan(a->max_contact_loss) || std::isnan(a->max_pen_loss) || std::isnan(a->max_total_loss))
        return fail(PARC_ERR_INVALID, "msel: run: a threshold is not a number (INFINITY switches one off)");
    const mpath::Scene &S = h->mpath->scene;
    if (S.N > h->max_rows) return fail(PARC_ERR_INVALID, "msel: run: the scene has more rows than the handle was made for");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const msel::Frames R{a->frames, a->final_frame, a->noise, a->num_frames, a->frame_stride};
    const int N = S.N, FD = h->FD;
    HIPCHK(hipEventRecord(h->ev[0], st));
    PARC_TRY(tool::launch(msel::k_msel_bounds, dim3((unsigned)N), dim3(msel::WV), 0, st, S, R, h->cfg, FD, a->slice_terrain != 0, h->W));
    HIPCHK(hipEventRecord(h->ev[1], st));
    PARC_TRY(tool::launch(msel::k_msel_fk, dim3(blocks((long long)N * a->num_frames, 64)), dim3(64), 0, st, h->d_model, R, N, FD, h->W));
    HIPCHK(hipEventRecord(h->ev[2], st));
    PARC_TRY(tool::launch(msel::k_msel_score, dim3((unsigned)((long long)N * a->num_frames)), dim3(msel::SC_THREADS), 0, st, h->d_model, S, R, h->cfg, FD, h->W));
    HIPCHK(hipEventRecord(h->ev[3], st));
    PARC_TRY(tool::launch(msel::k_msel_rank, dim3((unsigned)S.P), dim3(msel::WV), 0, st, S, R, h->cfg, a->max_contact_loss, a->max_pen_loss, a->max_total_loss, h->W));
    HIPCHK(hipEventRecord(h->ev[4], st));
    h->last_rows = N; h->last_P = S.P; h->last_X = S.X; h->last_Y = S.Y; h->last_launches = PARC_MSEL_RUN_LAUNCHES; h->ran = true; h->gathered = false;
    return PARC_OK;
}

static int msel_need_run(ParcPathSelect *h) {
    if (!h) return fail(PARC_ERR_INVALID, "msel: null argument");
    if (!h->ran) return fail(PARC_ERR_STATE, "msel: parc_msel_run first");
    const mpath::Scene &S = h->mpath->scene;   // the tables of the last run index a terrain of its dims
    if (!h->mpath->have_scene || S.N != h->last_rows || S.P != h->last_P || S.X != h->last_X || S.Y != h->last_Y)
        return fail(PARC_ERR_STATE, "msel: the scene changed since the last parc_msel_run");
    return PARC_OK;
}

static int msel_views(ParcPathSelect *h, hipStream_t st) {
    h->views.resize((size_t)h->last_rows);
    HIPCHK(hipMemcpyAsync(h->views.data(), h->W.view, h->views.size() * sizeof(msel::View), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PARC_OK;
}

extern "C" int parc_msel_results(ParcPathSelect *h, const ParcPathSelectResults *r, void *stream) {
    PARC_TRY(msel_need_run(h));
    if (!r) return fail(PARC_ERR_INVALID, "msel: null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)h->last_rows, P = (size_t)h->mpath->scene.P;
    const msel::Work &W = h->W;
    if (r->contact_loss) HIPCHK(hipMemcpyAsync(r->contact_loss, W.contact, N * sizeof(float), hipMemcpyDeviceToHost, st));
    if (r->pen_loss) HIPCHK(hipMemcpyAsync(r->pen_loss, W.pen, N * sizeof(float), hipMemcpyDeviceToHost, st));
    if (r->total_loss) HIPCHK(hipMemcpyAsync(r->total_loss, W.total, N * sizeof(float), hipMemcpyDeviceToHost, st));
    if (r->valid) HIPCHK(hipMemcpyAsync(r->valid, W.ok, N * sizeof(int), hipMemcpyDeviceToHost, st));
    if (r->order) HIPCHK(hipMemcpyAsync(r->order, W.order, N * sizeof(int), hipMemcpyDeviceToHost, st));
    if (r->num_valid) HIPCHK(hipMemcpyAsync(r->num_valid, W.num_valid, P * sizeof(int), hipMemcpyDeviceToHost, st));
    PARC_TRY(msel_views(h, st));
    for (size_t i = 0; i < N; ++i) {
        const msel::View &v = h->views[i];
        if (r->status) r->status[i] = v.status;
        if (r->num_frames) r->num_frames[i] = v.n;
        if (r->slice_min_point) { r->slice_min_point[2 * i] = v.mnx; r->slice_min_point[2 * i + 1] = v.mny; }
        if (r->slice_dims) { r->slice_dims[2 * i] = v.sx; r->slice_dims[2 * i + 1] = v.sy; }
    }
    return PARC_OK;
}

extern "C" int parc_msel_gather(ParcPathSelect *h, const int32_t *rows_host, int32_t count, float *hf_host, int64_t capacity, void *stream) {
    PARC_TRY(msel_need_run(h));
    if (count < 1 || !rows_host || !hf_host) return fail(PARC_ERR_INVALID, "msel: gather: count must be >= 1 with rows and an output given");
    for (int i = 0; i < count; ++i)
        if (rows_host[i] < 0 || rows_host[i] >= h->last_rows) return fail(PARC_ERR_INVALID, "msel: gather: rows[" + std::to_string(i) + "] is no row of the last run");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    PARC_TRY(msel_views(h, st));
    std::vector<long long> off((size_t)count);
    long long total = 0;                   // the host's scan of the named rows' dims; a row with a status bit has no cells
    for (int i = 0; i < count; ++i) {
        const msel::View &v = h->views[(size_t)rows_host[i]];
        off[(size_t)i] = total;
        total += v.status ? 0 : (long long)v.sx * v.sy;
    }
    if (total > capacity) return fail(PARC_ERR_INVALID, "msel: gather: capacity " + std::to_string(capacity) + " is below the " + std::to_string(total) + " cells of the rows");
    if (total == 0) return PARC_OK;
    DeviceArena tmp;                       // this call's
    int *d_rows = nullptr;
    long long *d_off = nullptr;
    float *d_out = nullptr;
    PARC_TRY(tmp.alloc(d_rows, count, rows_host));
    PARC_TRY(tmp.alloc(d_off, count, off.data()));
    PARC_TRY(tmp.alloc(d_out, total));
    HIPCHK(hipEventRecord(h->ev[5], st));
    PARC_TRY(tool::launch(msel::k_msel_gather, dim3((unsigned)count), dim3(256), 0, st, h->mpath->scene, h->W, d_rows, d_off, d_out));
    HIPCHK(hipEventRecord(h->ev[6], st));
    HIPCHK(hipMemcpyAsync(hf_host, d_out, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    h->gathered = true;
    return PARC_OK;
}

extern "C" int parc_msel_kernel_times(ParcPathSelect *h, float *ms5) {
    if (!h || !ms5) return fail(PARC_ERR_INVALID, "msel: null argument");
    const tool::Span spans[5] = {{h->ran, 0, 1}, {h->ran, 1, 2}, {h->ran, 2, 3}, {h->ran, 3, 4}, {h->gathered, 5, 6}};
    return tool::span_times("msel: no run yet", h->device, h->ev, spans, ms5);
}

extern "C" int parc_msel_describe(ParcPathSelect *h, int64_t *out6) {
    if (!h || !out6) return fail(PARC_ERR_INVALID, "msel: null argument");
    out6[0] = h->last_launches; out6[1] = h->max_rows; out6[2] = h->W.max_frames; out6[3] = PARC_MSEL_MAX_SLICE_DIM; out6[4] = h->host_model.P; out6[5] = h->last_rows;
    return PARC_OK;
}
