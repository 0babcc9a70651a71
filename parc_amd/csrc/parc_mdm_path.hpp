// parc_mdm_path.hpp — path-following motion generation on gfx950 (parc_mpath_*, include/parc_env.h): the world-frame wrapper
// of the motion generator (motion_generator/gen_util.py:27-153, RELATIVE_TO_ROOT) and the autoregressive rollout along a path
// (motion_synthesis/procgen/mdm_path.py:129-383), N rows at once, each on the terrain and the path of its row_path entry.
//   k_mpath_begin   once per rollout without given previous frames: the blank frames, the last one placed at node 0 (:150-167)
//   k_mpath_cond    a wave per row: closest node, target node, done, the canonical record, the 31 x 31 heights, the target direction, the
//                   previous frames canonicalised and standardised, the flags, x_T (drawn from the row's key, or copied)
//   k_mpath_append  a lane per (row, frame): un-standardise, exp map / dofs -> quaternions, un-canonicalise, store the window's range
//                   into the rollout buffer and the next window's previous frames
// Between the two, parc_mdm_sample as it is.  No float atomics and no reduction across rows; the rows not done are counted with one
// integer atomic per row, read back once per window.
#pragma once
#include "parc_mdm.hpp"
#include "parc_tool_handle.hpp"

namespace mpath {
using namespace parc;

constexpr int CW = 64;                     // k_mpath_cond: one wave; k_mpath_append / k_mpath_begin: lanes per block
constexpr int G = PARC_MDM_GRID;
constexpr int KEY_WINDOWS = 4096;          // x_T of window w of row id r: the draws of sample index r * KEY_WINDOWS + w, step 0
constexpr unsigned BEGIN_STEP = 0xFFFFFFu; // the step field of the begin kernel's draws (x_T is step 0, DDPM noise 1 ..)

struct Scene {                             // device pointers of one set_scene
    int P, X, Y, maxn, N;
    float dx, dy;
    const float *hf, *minp, *paths;        // [P][X][Y], [P][2], [P][maxn][3]
    const int *counts, *row_path;          // [P], [N]
};
struct Cfg {                               // by value
    int lookahead, lf, rf, target_flag, prev_flag;
    float max_h, done_radius;
    float gx[G], gy[G];                    // the local grid's coordinates (geom_util.get_xy_grid_points about the origin)
};
struct CondOut {
    float *hf, *target, *prev_state;       // ParcMdmConds' layout
    int *obs_flag, *target_flag, *prev_flag, *ind;
    int *done, *closest, *target_node;
    float *canon;                          // [N][8]: xy, z, heading, heading quaternion
};

// a frame of the rollout buffer: root position 3, root rotation 4, joint rotations (B - 1) x 4, contacts B
__host__ __device__ __forceinline__ int frame_floats(int B) { return 7 + 4 * (B - 1) + B; }

__global__ void __launch_bounds__(CW) k_mpath_begin(const CharTree *Mp, Scene S, int nprev, float *prev, const float *rel_h, const float *heading, int random_heading,
                                                    unsigned long long seed, const long long *path_ids) {
    const int B = Mp->B, FD = frame_floats(B);
    const long long i = (long long)blockIdx.x * CW + threadIdx.x;
    if (i >= (long long)S.N * nprev) return;
    const int row = (int)(i / nprev), f = (int)(i - (long long)row * nprev), p = S.row_path[row];
    float *o = prev + i * FD;
    for (int k = 0; k < FD; ++k) o[k] = 0.f;
    o[6] = 1.f;
    for (int j = 0; j < B - 1; ++j) o[7 + 4 * j + 3] = 1.f;
    if (f != nprev - 1) return;
    const float *n0 = S.paths + (size_t)p * S.maxn * 3;
    float u[4];
    philox4(seed, ((unsigned long long)BEGIN_STEP << 40) | (unsigned long long)path_ids[p], 0u, u);   // the path's id, not its place in the scene
    const float rel = rel_h ? rel_h[p] : u[0] * (0.9f - 0.7f) + 0.7f;
    float h;
    if (heading) h = heading[p];
    else if (random_heading) h = u[1] * 2.0f * 3.14159265358979323846f;
    else h = atan2f(n0[4] - n0[1], n0[3] - n0[0]);
    o[0] = n0[0]; o[1] = n0[1]; o[2] = n0[2] + rel;
    st4(o + 3, axis_angle_to_quat(mk3(0.f, 0.f, 1.f), h));
}

__global__ void __launch_bounds__(CW) k_mpath_cond(const mdm::Net *Np, const CharTree *Mp, Scene S, Cfg C, const float *prev, CondOut O, int first, int ind_val,
                                                   int *not_done, float *x, const float *noise, int draw, unsigned long long seed, const long long *row_ids,
                                                   unsigned window) {
    extern __shared__ float4 smem4[];
    const mdm::Net &N = *Np;
    const CharTree &M = *Mp;
    const int row = blockIdx.x, lane = threadIdx.x;
    const int B = M.B, J = B - 1, D = N.D, nprev = N.nprev, FD = frame_floats(B), per = (D + 11 * B) | 1;
    const int p = S.row_path[row], cnt = S.counts[p];
    const float *path = S.paths + (size_t)p * S.maxn * 3;
    const float *pf = prev + (size_t)row * nprev * FD, *last = pf + (size_t)(nprev - 1) * FD;
    // the canonical record (gen_util.py:49-54), the same in every lane
    const float cx = last[0], cy = last[1], cz = last[2];
    const float heading = calc_heading(ld4(last + 3));
    const Q4 hq = axis_angle_to_quat(mk3(0.f, 0.f, 1.f), heading), hqi = axis_angle_to_quat(mk3(0.f, 0.f, 1.f), -heading);
    // closest node (mdm_path.py:224-233), lowest index on ties
    float best = INFINITY;
    int bi = 0x7fffffff;
    for (int i = lane; i < cnt; i += CW) {
        const float ax = cx - path[3 * i], ay = cy - path[3 * i + 1], d2 = ax * ax + ay * ay;
        if (d2 < best) { best = d2; bi = i; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi >= cnt) bi = 0;                 // a non-finite root position compares with nothing
    const int tn = first ? 1 : min(bi + C.lookahead, cnt - 1);
    // lanes [0, nprev): the previous frames canonicalised, FK, features, standardised; lane nprev: FK of the last frame in the world (done)
    int done = 0;
    if (lane <= nprev) {
        float *fr = (float *)smem4 + (size_t)lane * per, *pos = fr + D, *rot = pos + 3 * B, *jr = rot + 4 * B;
        const float *src = lane < nprev ? pf + (size_t)lane * FD : last;
        for (int j = 1; j < B; ++j) st4(jr + 4 * j, ld4(src + 7 + 4 * (j - 1)));
        V3 rp = ld3(src);
        Q4 rr = ld4(src + 3);
        if (lane < nprev) {
            rp = quat_rotate(hqi, mk3(rp.x - cx, rp.y - cy, rp.z));
            rp.z = rp.z - cz;
            rr = quat_mul(hqi, rr);
        }
        fk_frame(M, rp, rr, jr, pos, rot);
        if (lane < nprev) {
            const int o_jp = 6, o_jr = 6 + 3 * J, o_c = o_jr + M.D;
            st3(fr, rp);
            st3(fr + 3, quat_to_exp_map(rr));
            for (int k = 0; k < 3 * J; ++k) fr[o_jp + k] = pos[3 + k];
            for (int j = 1; j < B; ++j) mdm::rot_to_dof(M, j, ld4(jr + 4 * j), fr + o_jr);
            for (int k = 0; k < B; ++k) fr[o_c + k] = src[7 + 4 * J + k];
            const float *mean = N.mean + (size_t)lane * D, *sd = N.std + (size_t)lane * D;
            float *o = O.prev_state + ((size_t)row * nprev + lane) * D;
            for (int k = 0; k < D; ++k) o[k] = (fr[k] - mean[k]) / sd[k];
        } else {
            const float *lf = pos + 3 * C.lf, *rf = pos + 3 * C.rf, *fin = path + 3 * (cnt - 1);
            const float ex = (lf[0] + rf[0]) / 2.0f - fin[0], ey = (lf[1] + rf[1]) / 2.0f - fin[1], ez = (lf[2] + rf[2]) / 2.0f - fin[2];
            done = sqrtf(ex * ex + ey * ey + ez * ez) < C.done_radius ? 1 : 0;
        }
    }
    done = __shfl(done, nprev, 64);
    // the heights (terrain_util.py:1949-1986): local grid rotated by the heading about the centre, round half to even, clamped to the grid
    const float ch = cosf(heading), sh = sinf(heading);
    const float minx = S.minp[2 * p], miny = S.minp[2 * p + 1];
    const float *hf = S.hf + (size_t)p * S.X * S.Y;
    for (int k = lane; k < G * G; k += CW) {
        const int ix = k / G, iy = k - ix * G;
        const float lx = C.gx[ix], ly = C.gy[iy];
        const float wx = (lx * ch - ly * sh) + cx, wy = (lx * sh + ly * ch) + cy;
        const float fx = rintf((wx - minx) / S.dx), fy = rintf((wy - miny) / S.dy);
        const int gx = (int)fminf(fmaxf(fx, 0.f), (float)(S.X - 1)), gy = (int)fminf(fmaxf(fy, 0.f), (float)(S.Y - 1));
        const float h = hf[(size_t)gx * S.Y + gy] - cz;
        O.hf[(size_t)row * G * G + k] = fminf(fmaxf(h, -C.max_h), C.max_h) / C.max_h;
    }
    if (x) {
        const int per_x = N.T * D;
        const unsigned long long idx = (unsigned long long)row_ids[row] * KEY_WINDOWS + window;
        for (int e = lane; e < per_x; e += CW)
            x[(size_t)row * per_x + e] = draw ? mdm::normal_at(seed, idx, 0u, (unsigned)e) : noise[(size_t)row * per_x + e];
    }
    if (lane == 0) {
        // the target (gen_util.py:94-96): F.normalize, eps 1e-12
        const float tx = path[3 * tn] - cx, ty = path[3 * tn + 1] - cy, a = -heading;
        const float ca = cosf(a), sa = sinf(a);
        const float ox = tx * ca - ty * sa, oy = tx * sa + ty * ca;
        const float nn = fmaxf(sqrtf(ox * ox + oy * oy), 1e-12f);
        O.target[2 * row] = ox / nn; O.target[2 * row + 1] = oy / nn;
        O.obs_flag[row] = 1; O.target_flag[row] = C.target_flag; O.prev_flag[row] = C.prev_flag; O.ind[row] = ind_val;
        O.done[row] = done; O.closest[row] = bi; O.target_node[row] = tn;
        float *c = O.canon + 8 * (size_t)row;
        c[0] = cx; c[1] = cy; c[2] = cz; c[3] = heading;
        st4(c + 4, hq);
        if (not_done && !done) atomicAdd(not_done, 1);
    }
}

// gen_sequence's torch.where and extract_motion_features (mdm.py:1153-1158), then gen_util.py:137-144.  Frames [lo, hi) of the window go
// to frames[row][off ..], frames [pn_lo, pn_hi) to prev_next; final_frame (total >= 0) takes `total` where the row is done for the first time.
__global__ void __launch_bounds__(CW) k_mpath_append(const mdm::Net *Np, const CharTree *Mp, int n, const float *x, const float *prevstd, const int *ind,
                                                     const float *canon, int guided, int lo, int hi, int off, float *frames, int max_frames, float *prev_next,
                                                     int pn_lo, int pn_hi, const int *done, int *final_frame, int total) {
    extern __shared__ float4 smem4[];
    const mdm::Net &N = *Np;
    const CharTree &M = *Mp;
    const int B = M.B, J = B - 1, D = N.D, T = N.T, nprev = N.nprev, FD = frame_floats(B), per = D | 1;
    const long long i = (long long)blockIdx.x * CW + threadIdx.x;
    if (i >= (long long)n * T) return;
    const int s = (int)(i / T), f = (int)(i - (long long)s * T);
    if (f == 0 && final_frame && total >= 0 && done[s] && final_frame[s] < 0) final_frame[s] = total;
    float *d0 = (frames && f >= lo && f < hi && off + f - lo < max_frames) ? frames + ((size_t)s * max_frames + off + f - lo) * FD : nullptr;
    float *d1 = (prev_next && f >= pn_lo && f < pn_hi) ? prev_next + ((size_t)s * (pn_hi - pn_lo) + f - pn_lo) * FD : nullptr;
    if (!d0 && !d1) return;
    const bool clean = f < nprev && ind[s] && !guided;
    const float *src = clean ? prevstd + ((size_t)s * nprev + f) * D : x + i * D;
    const float *mean = N.mean + (size_t)f * D, *sd = N.std + (size_t)f * D;
    float *fr = (float *)smem4 + (size_t)threadIdx.x * per;
    for (int k = 0; k < D; ++k) fr[k] = src[k] * sd[k] + mean[k];
    const float *c = canon + 8 * (size_t)s;
    const Q4 hq = ld4(c + 4);
    V3 wp = quat_rotate(hq, ld3(fr));
    wp.x = wp.x + c[0]; wp.y = wp.y + c[1]; wp.z = wp.z + c[2];
    const Q4 wq = quat_mul(hq, exp_map_to_quat(ld3(fr + 3)));
    const int o_jr = 6 + 3 * J, o_c = o_jr + M.D;
    float *dst[2] = {d0, d1};
    for (int t = 0; t < 2; ++t)
        if (dst[t]) { st3(dst[t], wp); st4(dst[t] + 3, wq); }
    for (int j = 1; j < B; ++j) {
        const Q4 q = dof_rot(M, j, fr + o_jr);
        if (d0) st4(d0 + 7 + 4 * (j - 1), q);
        if (d1) st4(d1 + 7 + 4 * (j - 1), q);
    }
    for (int k = 0; k < B; ++k) {
        if (d0) d0[7 + 4 * J + k] = fr[o_c + k];
        if (d1) d1[7 + 4 * J + k] = fr[o_c + k];
    }
}
}  // namespace mpath

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
// device: the generator's; ev: window w: 4 w .. 4 w + 3 (around k_mpath_cond, around k_mpath_append)
struct ParcMdmPath : tool::Handle<mdm::EventList> {
    ParcMdmPathParams params{};
    ParcMdm *mdm = nullptr;
    mpath::Cfg cfg{};
    int T = 0, nprev = 0, D = 0, B = 0, FD = 0, start = 0, step = 0, max_frames = 0, max_windows = 0, max_batch = 0;
    size_t lds_cond = 0, lds_app = 0;
    DeviceArena scene_mem;
    mpath::Scene scene{};
    bool have_scene = false, rolled = false;
    float *d_prev = nullptr, *d_prevstd = nullptr, *d_hf = nullptr, *d_target = nullptr, *d_canon = nullptr, *d_x = nullptr, *d_plan = nullptr;
    int *d_ints = nullptr, *d_counter = nullptr;   // d_ints: obs, target, prev flags, ind, done, closest, target node, [max_batch] each
    long long *d_row_ids = nullptr, *d_path_ids = nullptr;   // d_path_ids [P] lives with the scene
    int *h_counter = nullptr;                      // pinned
    std::vector<int> ts;
    int last_windows = 0, last_launches = 0, last_frames = 0;
    ~ParcMdmPath() { if (h_counter) (void)hipHostFree(h_counter); }
    mpath::CondOut own() const {
        const int mb = max_batch;
        return mpath::CondOut{d_hf, d_target, d_prevstd, d_ints, d_ints + mb, d_ints + 2 * mb, d_ints + 3 * mb, d_ints + 4 * mb, d_ints + 5 * mb, d_ints + 6 * mb, d_canon};
    }
};

extern "C" void parc_mpath_destroy(ParcMdmPath *h) { tool::destroy(h); }

extern "C" int parc_mpath_create(const ParcMdmPathParams *p, ParcMdmPath **out) {
    using namespace mpath;
    PARC_TRY(tool::create_args("mpath", "ParcMdmPathParams", p, out));
    if (!p->mdm) return fail(PARC_ERR_INVALID, "mpath: mdm is null (the generator the rollout drives)");
    ParcMdm *g = p->mdm;
    const int T = g->net.T, nprev = g->net.nprev, B = g->host_model.B;
    if (nprev < 1 || nprev >= mpath::CW)
        return fail(PARC_ERR_INVALID, "mpath: num_prev_states must be 1 .. 63 (the canonical frame is the last previous frame; k_mpath_cond gives every previous frame a lane and one more to the done test)");
    if (1 + p->num_x_neg + p->num_x_pos != G || 1 + p->num_y_neg + p->num_y_pos != G || p->num_x_neg < 0 || p->num_y_neg < 0)
        return fail(PARC_ERR_INVALID, "mpath: heightmap.local_grid must be 31 x 31 points");
    if (!(p->grid_dx > 0.f) || !(p->grid_dy > 0.f) || !std::isfinite(p->grid_dx) || !std::isfinite(p->grid_dy)) return fail(PARC_ERR_INVALID, "mpath: heightmap.horizontal_scale must be positive");
    if (!(p->max_h > 0.f) || !std::isfinite(p->max_h)) return fail(PARC_ERR_INVALID, "mpath: heightmap.max_h must be positive");
    if (p->next_node_lookahead < 0) return fail(PARC_ERR_INVALID, "mpath: next_node_lookahead must be >= 0");
    const int start = T - 1 - p->rewind_num_frames;
    if (p->rewind_num_frames < 0 || start - nprev < 1)
        return fail(PARC_ERR_INVALID, "mpath: rewind_num_frames must leave seq_len - 1 - rewind_num_frames - num_prev_states >= 1 new frames per window");
    if (!(p->max_motion_length > 0.f) || !std::isfinite(p->max_motion_length)) return fail(PARC_ERR_INVALID, "mpath: max_motion_length must be positive");
    if (!(p->sequence_fps > 0.f) || !std::isfinite(p->sequence_fps)) return fail(PARC_ERR_INVALID, "mpath: sequence_fps must be positive");
    if (!p->use_ddim) return fail(PARC_ERR_INVALID, "mpath: use_ddim must be true (the rollout samples with DDIM)");
    if (p->ddim_stride < 1 || p->ddim_stride > g->params.diffusion_timesteps) return fail(PARC_ERR_INVALID, "mpath: ddim_stride must be 1 .. diffusion_timesteps");
    if (!std::isfinite(p->cfg_scale)) return fail(PARC_ERR_INVALID, "mpath: cfg_scale must be finite");
    if (p->left_foot < 0 || p->left_foot >= B || p->right_foot < 0 || p->right_foot >= B) return fail(PARC_ERR_INVALID, "mpath: left_foot / right_foot body id out of range");
    // the longest rollout (mdm_path.py:340-377): windows until total * dt > max_motion_length, the last one kept to its end
    const int step = start - nprev;
    const double dt = 1.0 / (double)p->sequence_fps;
    long long total = start;
    int W = 1;
    for (;;) {
        total += step; ++W;
        if ((double)total * dt > (double)p->max_motion_length) break;
        if (W >= KEY_WINDOWS) return fail(PARC_ERR_INVALID, "mpath: max_motion_length needs more than " + std::to_string(KEY_WINDOWS) + " windows");
    }
    std::vector<int> ts;
    for (int t = 0; t < g->params.diffusion_timesteps; t += p->ddim_stride) ts.insert(ts.begin(), t);   // reversed(range(0, timesteps, stride))
    if ((int)ts.size() > PARC_MDM_MAX_STEPS) return fail(PARC_ERR_INVALID, "mpath: ddim_stride gives more than PARC_MDM_MAX_STEPS steps");
    return tool::create("mpath", g->device, out, [&](ParcMdmPath &h) -> int {
        h.params = *p; h.mdm = g; h.ts = ts;
        h.T = T; h.nprev = nprev; h.D = g->net.D; h.B = B; h.FD = frame_floats(B); h.start = start; h.step = step; h.max_batch = g->params.max_batch;
        h.max_windows = W;
        h.max_frames = start + (W - 2) * step + (T - nprev);
        Cfg &c = h.cfg;
        c.lookahead = p->next_node_lookahead; c.lf = p->left_foot; c.rf = p->right_foot;
        c.target_flag = p->target_condition_key != 0; c.prev_flag = p->prev_state_ind_key != 0; c.max_h = p->max_h; c.done_radius = 0.5f;
        // torch.linspace(-d n_neg, d n_pos, 31) in fp32: start + step i below the middle, end - step (30 - i) from it on
        auto linspace = [](float d, int nneg, int npos, float *o) {
            const float a = 0.f - (float)((double)d * nneg), b = 0.f + (float)((double)d * npos), st = (b - a) / (float)(G - 1);
            for (int i = 0; i < G; ++i) o[i] = i < G / 2 ? a + st * (float)i : b - st * (float)(G - 1 - i);
        };
        linspace(p->grid_dx, p->num_x_neg, p->num_x_pos, c.gx);
        linspace(p->grid_dy, p->num_y_neg, p->num_y_pos, c.gy);
        const long long mb = h.max_batch;
        PARC_TRY(h.mem.alloc_fill(h.d_prev, mb * nprev * h.FD));
        PARC_TRY(h.mem.alloc_fill(h.d_prevstd, mb * nprev * h.D));
        PARC_TRY(h.mem.alloc_fill(h.d_hf, mb * G * G));
        PARC_TRY(h.mem.alloc_fill(h.d_target, mb * 2));
        PARC_TRY(h.mem.alloc_fill(h.d_canon, mb * 8));
        PARC_TRY(h.mem.alloc_fill(h.d_x, mb * T * h.D));
        PARC_TRY(h.mem.alloc_fill(h.d_ints, mb * 7));
        PARC_TRY(h.mem.alloc_fill(h.d_counter, h.max_windows));
        PARC_TRY(h.mem.alloc_fill(h.d_row_ids, mb));
        HIPCHK(hipHostMalloc((void **)&h.h_counter, sizeof(int)));
        h.lds_cond = (size_t)(nprev + 1) * ((h.D + 11 * B) | 1) * sizeof(float);
        h.lds_app = (size_t)CW * (h.D | 1) * sizeof(float);
        if (h.lds_cond > 160 * 1024) return fail(PARC_ERR_INVALID, "mpath: num_prev_states too large for the conditions kernel's LDS");
        HIPCHK(hipFuncSetAttribute((const void *)k_mpath_cond, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h.lds_cond));
        HIPCHK(hipFuncSetAttribute((const void *)k_mpath_append, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h.lds_app));
        return h.ev.ensure(4);
    });
}

extern "C" int parc_mpath_set_scene(ParcMdmPath *h, const float *hf_host, int32_t num_terrains, int32_t dim_x, int32_t dim_y, const float *min_points_host, float dx,
                                    float dy, const float *paths_host, const int32_t *path_counts_host, int32_t max_nodes, const int32_t *row_path_host,
                                    int32_t num_rows) {
    if (!h) return fail(PARC_ERR_INVALID, "mpath: null argument");
    if (!hf_host || !min_points_host || !paths_host || !path_counts_host || !row_path_host) return fail(PARC_ERR_INVALID, "mpath: set_scene: null array");
    if (num_terrains < 1 || dim_x < 1 || dim_y < 1) return fail(PARC_ERR_INVALID, "mpath: set_scene: the terrains must be [P >= 1][X >= 1][Y >= 1]");
    if (!(dx > 0.f) || !(dy > 0.f) || !std::isfinite(dx) || !std::isfinite(dy)) return fail(PARC_ERR_INVALID, "mpath: set_scene: dx / dy must be positive");
    if (num_rows < 1 || num_rows > h->max_batch) return fail(PARC_ERR_INVALID, "mpath: set_scene: the rows must be 1 .. the generator's max_batch = " + std::to_string(h->max_batch));
    if (max_nodes < 2) return fail(PARC_ERR_INVALID, "mpath: set_scene: max_nodes must be >= 2");
    const long long P = num_terrains;
    for (long long i = 0; i < P * dim_x * dim_y; ++i)
        if (!std::isfinite(hf_host[i])) return fail(PARC_ERR_INVALID, "mpath: set_scene: a terrain height is not finite");
    for (long long i = 0; i < 2 * P; ++i)
        if (!std::isfinite(min_points_host[i])) return fail(PARC_ERR_INVALID, "mpath: set_scene: a min_point is not finite");
    for (long long p = 0; p < P; ++p) {
        const int c = path_counts_host[p];
        if (c < 2 || c > max_nodes) return fail(PARC_ERR_INVALID, "mpath: set_scene: path " + std::to_string(p) + " has " + std::to_string(c) + " nodes; a path has 2 .. max_nodes");
        for (long long i = 0; i < 3LL * c; ++i)
            if (!std::isfinite(paths_host[p * max_nodes * 3 + i])) return fail(PARC_ERR_INVALID, "mpath: set_scene: path " + std::to_string(p) + " has a non-finite node");
    }
    for (int r = 0; r < num_rows; ++r)
        if (row_path_host[r] < 0 || row_path_host[r] >= num_terrains) return fail(PARC_ERR_INVALID, "mpath: set_scene: row_path[" + std::to_string(r) + "] is no path of the scene");
    HIPCHK(hipSetDevice(h->device));
    DeviceArena a;
    mpath::Scene S{};
    S.P = num_terrains; S.X = dim_x; S.Y = dim_y; S.maxn = max_nodes; S.N = num_rows; S.dx = dx; S.dy = dy;
    float *f = nullptr;
    int *ip = nullptr;
    PARC_TRY(a.alloc(f, P * dim_x * dim_y, hf_host)); S.hf = f;
    PARC_TRY(a.alloc(f, 2 * P, min_points_host)); S.minp = f;
    PARC_TRY(a.alloc(f, P * max_nodes * 3, paths_host)); S.paths = f;
    PARC_TRY(a.alloc(ip, P, path_counts_host)); S.counts = ip;
    PARC_TRY(a.alloc(ip, num_rows, row_path_host)); S.row_path = ip;
    float *plan = nullptr;
    long long *pids = nullptr;
    PARC_TRY(a.alloc(plan, 2 * P));
    PARC_TRY(a.alloc(pids, P));
    HIPCHK(hipDeviceSynchronize());   // a rollout in flight reads the scene it was given
    h->scene_mem.swap(a);
    h->d_plan = plan; h->d_path_ids = pids;
    h->scene = S; h->have_scene = true;
    return PARC_OK;
}

static int mpath_launch_cond(ParcMdmPath *h, const float *prev, const mpath::CondOut &O, int first, int ind_val, int *not_done, float *x, const float *noise, int draw,
                             uint64_t seed, unsigned window, hipStream_t st) {
    PARC_TRY(tool::launch(mpath::k_mpath_cond, dim3((unsigned)h->scene.N), dim3(mpath::CW), h->lds_cond, st, h->mdm->d_net, h->mdm->d_model, h->scene, h->cfg, prev, O, first,
                       ind_val, not_done, x, noise, draw, (unsigned long long)seed, h->d_row_ids, window));
    return PARC_OK;
}

static int mpath_launch_append(ParcMdmPath *h, int n, const float *x, const float *prevstd, const int *ind, const float *canon, int guided, int lo, int hi, int off,
                               float *frames, int max_frames, float *prev_next, const int *done, int *final_frame, int total, hipStream_t st) {
    PARC_TRY(tool::launch(mpath::k_mpath_append, dim3(blocks((long long)n * h->T, mpath::CW)), dim3(mpath::CW), h->lds_app, st, h->mdm->d_net, h->mdm->d_model, n, x, prevstd,
                       ind, canon, guided, lo, hi, off, frames, max_frames, prev_next, h->start - h->nprev, h->start, done, final_frame, total));
    return PARC_OK;
}

extern "C" int parc_mpath_conds(ParcMdmPath *h, const float *prev_frames, int32_t first, int32_t blank, const ParcMdmPathCondOut *o, void *stream) {
    if (!h || !o) return fail(PARC_ERR_INVALID, "mpath: null argument");
    if (!h->have_scene) return fail(PARC_ERR_STATE, "mpath: parc_mpath_set_scene first");
    if (!prev_frames || !o->hf || !o->target || !o->prev_state || !o->obs_flag || !o->target_flag || !o->prev_state_flag || !o->noise_ind || !o->done || !o->closest_node ||
        !o->target_node || !o->canon)
        return fail(PARC_ERR_INVALID, "mpath: conds: null array");
    HIPCHK(hipSetDevice(h->device));
    const mpath::CondOut O{o->hf, o->target, o->prev_state, o->obs_flag, o->target_flag, o->prev_state_flag, o->noise_ind, o->done, o->closest_node, o->target_node, o->canon};
    const int ind_val = blank ? 0 : (first ? 1 : (h->params.use_prev_state != 0));   // given frames at the path's start force it on (mdm_path.py:169)
    return mpath_launch_cond(h, prev_frames, O, first != 0, ind_val, nullptr, nullptr, nullptr, 0, 0, 0u, (hipStream_t)stream);
}

extern "C" int parc_mpath_append(ParcMdmPath *h, const ParcMdmPathAppendArgs *a, void *stream) {
    if (!h || !a) return fail(PARC_ERR_INVALID, "mpath: null argument");
    if (!a->x || !a->prev_state || !a->noise_ind || !a->canon || !a->frames) return fail(PARC_ERR_INVALID, "mpath: append: null array");
    if (a->n < 1 || a->n > h->max_batch) return fail(PARC_ERR_INVALID, "mpath: append: n must be 1 .. the generator's max_batch = " + std::to_string(h->max_batch));
    if (a->lo < 0 || a->hi > h->T || a->lo > a->hi) return fail(PARC_ERR_INVALID, "mpath: append: the frame range must lie in 0 .. seq_len");
    if (a->offset < 0 || a->max_frames < 1 || a->offset + (a->hi - a->lo) > a->max_frames) return fail(PARC_ERR_INVALID, "mpath: append: offset + frames exceeds max_frames");
    if ((a->final_frame != nullptr) != (a->done != nullptr)) return fail(PARC_ERR_INVALID, "mpath: append: done and final_frame go together");
    HIPCHK(hipSetDevice(h->device));
    return mpath_launch_append(h, a->n, a->x, a->prev_state, a->noise_ind, a->canon, a->guided != 0, a->lo, a->hi, a->offset, a->frames, a->max_frames, a->prev_next, a->done,
                               a->final_frame, a->final_frame ? a->total : -1, (hipStream_t)stream);
}

extern "C" int parc_mpath_rollout(ParcMdmPath *h, const ParcMdmPathRolloutArgs *a, void *stream) {
    if (!h || !a) return fail(PARC_ERR_INVALID, "mpath: null argument");
    if (!h->have_scene) return fail(PARC_ERR_STATE, "mpath: parc_mpath_set_scene first");
    if (!a->frames || !a->final_frame || !a->done) return fail(PARC_ERR_INVALID, "mpath: rollout: null output array");
    if (a->noise && a->noise_windows < 1) return fail(PARC_ERR_INVALID, "mpath: rollout: noise_windows must be >= 1 with injected noise");
    if (a->heading_mode != PARC_MPATH_HEADING_AUTO && a->heading_mode != PARC_MPATH_HEADING_RANDOM) return fail(PARC_ERR_INVALID, "mpath: rollout: heading_mode must be auto or random");
    const int n = h->scene.N, T = h->T, nprev = h->nprev;
    for (int r = 0; r < n; ++r)
        if (a->row_ids_host && (a->row_ids_host[r] < 0 || a->row_ids_host[r] >= (1LL << 28))) return fail(PARC_ERR_INVALID, "mpath: rollout: row_ids must be 0 .. 2^28 - 1");
    for (int q = 0; q < h->scene.P; ++q)
        if (a->path_ids_host && (a->path_ids_host[q] < 0 || a->path_ids_host[q] >= (1LL << 40))) return fail(PARC_ERR_INVALID, "mpath: rollout: path_ids must be 0 .. 2^40 - 1");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    std::vector<long long> ids((size_t)n);
    for (int r = 0; r < n; ++r) ids[(size_t)r] = a->row_ids_host ? a->row_ids_host[r] : r;
    std::vector<long long> pids((size_t)h->scene.P);
    for (int q = 0; q < h->scene.P; ++q) pids[(size_t)q] = a->path_ids_host ? a->path_ids_host[q] : q;
    HIPCHK(hipMemcpyAsync(h->d_path_ids, pids.data(), pids.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->d_row_ids, ids.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));          // ids is this call's
    HIPCHK(hipMemsetAsync(h->d_counter, 0, (size_t)h->max_windows * sizeof(int), st));
    HIPCHK(hipMemsetAsync(a->final_frame, 0xFF, (size_t)n * sizeof(int), st));   // -1
    int launches = 0;
    const bool blank = a->prev_frames == nullptr;
    if (blank) {
        float *rel = nullptr, *head = nullptr;
        if (a->rel_height_host) { rel = h->d_plan; HIPCHK(hipMemcpyAsync(rel, a->rel_height_host, (size_t)h->scene.P * sizeof(float), hipMemcpyHostToDevice, st)); }
        if (a->heading_host) { head = h->d_plan + h->scene.P; HIPCHK(hipMemcpyAsync(head, a->heading_host, (size_t)h->scene.P * sizeof(float), hipMemcpyHostToDevice, st)); }
        if (rel || head) HIPCHK(hipStreamSynchronize(st));
        PARC_TRY(tool::launch(mpath::k_mpath_begin, dim3(blocks((long long)n * nprev, mpath::CW)), dim3(mpath::CW), 0, st, h->mdm->d_model, h->scene, nprev, h->d_prev, rel, head,
                           a->heading_mode == PARC_MPATH_HEADING_RANDOM, (unsigned long long)a->seed, h->d_path_ids));
        ++launches;
    } else
        HIPCHK(hipMemcpyAsync(h->d_prev, a->prev_frames, (size_t)n * nprev * h->FD * sizeof(float), hipMemcpyDeviceToDevice, st));
    const mpath::CondOut O = h->own();
    ParcMdmConds C{};
    C.n = n; C.hf = O.hf; C.target = O.target; C.prev_state = O.prev_state; C.obs_flag = O.obs_flag; C.target_flag = O.target_flag; C.prev_state_flag = O.prev_flag;
    C.noise_ind = O.ind;
    ParcMdmSampleArgs S{};
    S.mode = PARC_MDM_DDIM; S.num_steps = (int)h->ts.size(); S.timesteps_host = h->ts.data(); S.stride = h->params.ddim_stride; S.x = h->d_x;
    S.guidance_scale = h->params.cfg_scale;
    const long long per = (long long)n * T * h->D;
    const double dt = 1.0 / (double)h->params.sequence_fps;
    int total = h->start, count = 0, w = 0;
    for (;; ++w) {
        if (a->noise && w >= a->noise_windows) return fail(PARC_ERR_INVALID, "mpath: rollout: the injected noise holds " + std::to_string(a->noise_windows) + " windows, the rollout needs more");
        PARC_TRY(h->ev.ensure(4 * (size_t)(w + 1)));
        const bool first = w == 0;
        const int ind_val = (first && blank) ? 0 : (first ? 1 : (h->params.use_prev_state != 0));
        const int guided = (first && blank) ? 0 : (h->params.use_cfg != 0);
        HIPCHK(hipEventRecord(h->ev[4 * w], st));
        PARC_TRY(mpath_launch_cond(h, h->d_prev, O, first, ind_val, first ? nullptr : h->d_counter + w, h->d_x, a->noise ? a->noise + (long long)w * per : nullptr, a->noise == nullptr,
                                   a->seed, (unsigned)w, st));
        HIPCHK(hipEventRecord(h->ev[4 * w + 1], st));
        S.use_guidance = guided;
        PARC_TRY(parc_mdm_sample(h->mdm, &C, &S, stream));
        launches += 3 + 2 * S.num_steps;   // cond, the sampler's 1 + 2 steps, append
        bool last = false, all_done = false;
        if (!first) {                          // the one value the host reads per window: the rows not done
            HIPCHK(hipMemcpyAsync(h->h_counter, h->d_counter + w, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            total += h->step;
            all_done = *h->h_counter == 0;
            last = all_done || (double)total * dt > (double)h->params.max_motion_length;
        }
        const int lo = first ? 0 : nprev, hi = first ? h->start : (last ? T : h->start);
        HIPCHK(hipEventRecord(h->ev[4 * w + 2], st));
        PARC_TRY(mpath_launch_append(h, n, h->d_x, O.prev_state, O.ind, O.canon, guided, lo, hi, count, a->frames, h->max_frames, h->d_prev, O.done, a->final_frame,
                                     (!first && !all_done) ? total : -1, st));
        HIPCHK(hipEventRecord(h->ev[4 * w + 3], st));
        count += hi - lo;
        if (last) break;
    }
    HIPCHK(hipMemcpyAsync(a->done, O.done, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st));
    h->last_windows = w + 1; h->last_launches = launches; h->last_frames = count; h->rolled = true;
    return PARC_OK;
}

extern "C" int parc_mpath_kernel_times(ParcMdmPath *h, float *ms2) {
    if (!h || !ms2) return fail(PARC_ERR_INVALID, "mpath: null argument");
    if (!h->rolled) return fail(PARC_ERR_STATE, "mpath: no rollout yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev[4 * h->last_windows - 1]));
    ms2[0] = ms2[1] = 0.f;
    for (int w = 0; w < h->last_windows; ++w) {
        float a = 0.f, b = 0.f;
        PARC_TRY(h->ev.elapsed(a, 4 * w, 4 * w + 1));
        PARC_TRY(h->ev.elapsed(b, 4 * w + 2, 4 * w + 3));
        ms2[0] += a; ms2[1] += b;
    }
    return PARC_OK;
}

extern "C" int parc_mpath_describe(ParcMdmPath *h, int64_t *out6) {
    if (!h || !out6) return fail(PARC_ERR_INVALID, "mpath: null argument");
    out6[0] = h->max_frames; out6[1] = h->max_windows; out6[2] = h->FD; out6[3] = h->last_windows; out6[4] = h->last_launches; out6[5] = h->last_frames;
    return PARC_OK;
}
