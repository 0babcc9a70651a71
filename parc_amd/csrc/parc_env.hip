// parc_env.hip — the host side of the env: the ParcEnv handle, the parc_env_* C-ABI of include/parc_env.h and the launch helpers.  Its
// gfx950 kernels are in the headers below, one per seam (step path, curriculum, resets, operators, renderer), built from
// parc_env_tables.hpp.
// One of the library's three translation units: the rigid-body dynamics kernels are parc_dynamics.hip, seen from here through
// parc_dynamics_host.hpp alone; the stage-2 motion tools (parc_mopt_*, parc_mterr_*, parc_msamp_*, parc_pathplan_*, parc_tgen_*) and the
// learner's kernels are parc_tools.hip; what more than one unit uses is parc_common.hpp.
//
// Reference semantics: file:line citations relative to /root/reference.
// Every header includes what it uses; the order below does not matter.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"          // what this unit shares with the other two: g_err / fail / HIPCHK, DeviceArena, MotionMeta
#include "parc_dynamics_host.hpp"   // the dynamics step, as an opaque handle
#include "parc_env_tables.hpp"      // DevTables, StepParams, REC_*: what the kernels below and this file share
#include "parc_env_post.hpp"        // k_env_prep, k_env_post: observation, reward, done
#include "parc_curriculum.hpp"      // the done list and the fail-rate EMA that close a step
#include "parc_reset.hpp"           // k_reset_with, k_build_cdf
#include "parc_env_ops.hpp"         // k_motion_prep, the one-thread-per-item operators, the recorder, parc_test_quat_op's kernel
#include "parc_lanetab.hpp"         // parc_lanetab_fill, parc_hrot_fill: the per-lane tables of k_env_post
#include "parc_render.hpp"          // k_render (parc_env_render)
#include "parc_render_scene.hpp"    // parc_env_render_scene: the bins and k_render_scene
#include "parc_rowmap.hpp"          // parc_rowmap_mul: the row items of the lane table

struct ParcEnv {
    ParcEnvConfig cfg;
    int B, J, D, K, S, R, N, M = 0, T = 1;
    int obs_dim;
    int64_t F = 0;
    bool bound = false, have_motions = false, have_terrain = false;
    bool done_list_fresh = false;     // a step has produced a done list that parc_env_reset_done has not consumed yet
    // The device memory of the handle, one arena per lifetime; the d_* members below are views into them.
    DeviceArena mem;                  // create .. destroy: tables, prep records, done lists, render geoms
    DeviceArena motions;              // parc_env_load_motions: d_records, d_meta, d_weights, d_fail, d_cdf, d_motion_done
    DeviceArena terrain;              // parc_env_load_terrain: d_hf, d_motion_off
    DeviceArena scene;                // d_scene alone: released and allocated anew when it must grow
    StepParams sp;
    float4 *d_prep = nullptr;
    std::string dev_options_s, describe_s; // the dev_options this handle was created with (owned copy) / parc_env_describe
    unsigned int *h_health = nullptr, *d_health = nullptr; // two words of host-mapped pinned memory (publish_health) and their device alias
    HealthOut health = {nullptr, {nullptr, nullptr}};      // what the curriculum kernels publish: set when the dynamics run and d_health exists
    ParcDyn *dyn = nullptr;           // owned; the dynamics step (parc_dynamics_host.hpp), null when cfg.enable_dynamics is 0.  Same lifetime as `mem`
    DevTables h_tab;
    DevTables *d_tab = nullptr;
    unsigned row_mul = 0;  // j / (B - 1) == (j * row_mul) >> 16 for every joint item j (parc_rowmap.hpp, checked at create): host only, what
                           // both fills of the lane table (create, parc_env_load_terrain) form the row items with
    float *d_ray = nullptr, *d_env_off = nullptr, *d_hf = nullptr, *d_motion_off = nullptr;
    float4 *d_records = nullptr;
    MotionMeta *d_meta = nullptr;
    std::vector<MotionMeta> h_meta;
    std::vector<float> h_weights;
    float *d_weights = nullptr, *d_fail = nullptr, *d_cdf = nullptr;
    unsigned char *d_ema = nullptr;
    int *d_done_list = nullptr, *d_done_key = nullptr, *d_chunk_count = nullptr, *d_motion_done = nullptr, *d_reset_count = nullptr;
    int nchunks = 0;
    float *d_scratch_jr = nullptr;
    float *d_start_frac = nullptr;                 // parc_env_set_start_time_fraction (caller-owned)
    RenderGeoms *d_rgeom = nullptr;                // parc_env_render: the collision geoms, uploaded at creation
    float hf_max = 0.f;                            // highest column top (parc_env_load_terrain), bounds the renderer's terrain traversal
    float hf_min = 0.f;                            // lowest column top: the floor of the scene render's shadow-caster cull
    char *d_scene = nullptr;                       // parc_env_render_scene workspace, grown on demand (scene_ws_bytes), a view into `scene`
    int scene_cap = 0;                             // envs the workspace holds
    unsigned long long *d_reset_calls = nullptr;   // device counter of sampling resets (Philox call index)
    const float *action_bound = nullptr;           // parc_env_bind_action (caller-owned)
    hipGraphExec_t graph_exec = nullptr;           // parc_env_step_reset_graph
    bool graph_dirty = true;                       // StepParams travels by value with every launch; a captured graph holds a copy
    bool force_ema_leader = false;                 // test switch PARC_EMA_LEADER=1: the large-library EMA path on a small library
    bool force_two_launch_curriculum = false;      // test switch PARC_CURRICULUM_TWO_LAUNCHES=1: k_done_scatter + k_fail_rate_ema on a small shard
    int grid_waves = 0;
    int num_cus = 256;
    size_t lds_bytes = 0;
    float last_dyn_ms = 0.f;
    DeviceEvents<4> ev;
    float *rec_frames = nullptr, *rec_obs = nullptr;   // recorder ring buffers (caller-owned)
    int rec_cap = 0, rec_ref = 0;
    int *rec_count = nullptr, *rec_nwriting = nullptr;
    unsigned char *rec_writing = nullptr;
    bool timing = false;               // parc_env_set_kernel_timing: record events around the kernels of every step
    std::vector<hipEvent_t> tev;       // 4 events per timed step (step_sequence: before dynamics, after dynamics, after the obs kernels, after the curriculum)
    size_t tev_used = 0;

    ParcEnv() = default;
    ParcEnv(const ParcEnv &) = delete;
    ParcEnv &operator=(const ParcEnv &) = delete;
    ~ParcEnv() {
        (void)hipSetDevice(cfg.device);
        parc_dyn_destroy(dyn);
        mem.release(); motions.release(); terrain.release(); scene.release();
        if (h_health) (void)hipHostFree(h_health);
        for (hipEvent_t x : tev) if (x) (void)hipEventDestroy(x);
        if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    }
};

extern "C" const char *parc_last_error(void) { return g_err.c_str(); }
extern "C" int parc_abi_version(void) { return PARC_ABI_VERSION; }

extern "C" int parc_env_create(const ParcEnvConfig *cfg, ParcEnv **out) {
    if (!cfg || !out) return fail(PARC_ERR_INVALID, "null argument");
    if (cfg->abi_version != PARC_ABI_VERSION || cfg->struct_size != sizeof(ParcEnvConfig))
        return fail(PARC_ERR_INVALID, "ParcEnvConfig ABI mismatch (abi_version / struct_size)");
    const ParcCharModel &m = cfg->model;
    if (m.num_bodies < 2 || m.num_bodies > 15) return fail(PARC_ERR_INVALID, "num_bodies must be in [2,15]");
    if (m.dof_size < 1 || m.dof_size > PARC_MAX_DOFS) return fail(PARC_ERR_INVALID, "dof_size must be in [1,40]");
    if (cfg->num_tar_obs_steps < 1 || cfg->num_tar_obs_steps > PARC_MAX_TAR_STEPS) return fail(PARC_ERR_INVALID, "tar_obs_steps: 1..6 entries");
    if (cfg->num_key_bodies < 0 || cfg->num_key_bodies > PARC_MAX_KEY_BODIES) return fail(PARC_ERR_INVALID, "key_bodies: at most 8");
    if (cfg->num_envs < 1) return fail(PARC_ERR_INVALID, "num_envs must be >= 1");
    if (cfg->num_envs > 1024 * 1024) return fail(PARC_ERR_INVALID, "num_envs must be <= 1048576 per handle"); // 1024 chunks of 1024 (d_chunk_count)
    if (cfg->num_rays < 1 || cfg->num_rays > 4096 || !cfg->ray_points_host) return fail(PARC_ERR_INVALID, "ray fan: 1..4096 points");
    if (!cfg->env_offsets_host) return fail(PARC_ERR_INVALID, "env_offsets_host is required");
    for (int b = 1; b < m.num_bodies; ++b)
        if (m.parent[b] < 0 || m.parent[b] >= b) return fail(PARC_ERR_INVALID, "bodies must be in DFS order (parent < child)");
    if (cfg->enable_dynamics && !cfg->body_pos_from_fk)
        return fail(PARC_ERR_INVALID, "enable_dynamics needs body_pos_from_fk = 1 (the simulator is reduced-coordinate)");
    if (cfg->enable_dynamics && (cfg->dynamics.num_geoms < 1 || cfg->dynamics.num_geoms > PARC_MAX_GEOMS || !(cfg->dynamics.sim_dt > 0.f)))
        return fail(PARC_ERR_INVALID, "enable_dynamics: bad ParcDynamicsParams");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PARC_ERR_NO_DEVICE, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PARC_ERR_INVALID, "device ordinal out of range");
    HIPCHK(hipSetDevice(cfg->device));

    std::unique_ptr<ParcEnv> e(new (std::nothrow) ParcEnv()); // every failure below is a plain return: ~ParcEnv releases what exists
    if (!e) return fail(PARC_ERR_INVALID, "out of host memory");
    e->cfg = *cfg;
    e->dev_options_s = cfg->dev_options ? cfg->dev_options : "";
    e->cfg.dev_options = e->dev_options_s.c_str();
    e->cfg.ray_points_host = nullptr; e->cfg.env_offsets_host = nullptr;
    e->B = m.num_bodies; e->J = e->B - 1; e->D = m.dof_size; e->K = cfg->num_key_bodies; e->S = cfg->num_tar_obs_steps;
    e->R = cfg->num_rays; e->N = cfg->num_envs;
    const int B = e->B, J = e->J, D = e->D, K = e->K, S = e->S, R = e->R;

    DevTables &t = e->h_tab;
    memset(&t, 0, sizeof(t));
    for (int b = 0; b < 16; ++b) { t.h.parent[b] = -1; t.h.jtype[b] = PARC_JOINT_FIXED; t.h.key_slot[b] = -1; }
    for (int b = 0; b < B; ++b) {
        t.h.parent[b] = m.parent[b]; t.h.jtype[b] = m.joint_type[b]; t.h.dof_idx[b] = m.dof_idx[b];
        for (int c = 0; c < 3; ++c) { t.h.axis[b][c] = m.joint_axis[b][c]; t.h.lt[b][c] = m.local_translation[b][c]; }
        for (int c = 0; c < 4; ++c) t.h.lr[b][c] = m.local_rotation[b][c];
    }
    for (int p = 0; p < PARC_MAX_FK_PATHS; ++p)
        for (int d = 0; d < PARC_MAX_FK_DEPTH; ++d) {
            t.h.fk_paths[p][d] = m.fk_paths[p][d];
            if (m.fk_paths[p][d] >= B) return fail(PARC_ERR_INVALID, "fk_paths entry out of range");
        }
    const float dt_f = (float)cfg->control_dt;
    for (int s = 0; s < S; ++s) t.tstep[s] = dt_f * (float)cfg->tar_obs_steps[s];
    for (int k = 0; k < K; ++k) {
        if (cfg->key_body_ids[k] < 0 || cfg->key_body_ids[k] >= B) return fail(PARC_ERR_INVALID, "key body id out of range");
        t.h.key_ids[k] = cfg->key_body_ids[k];
        if (t.h.key_slot[cfg->key_body_ids[k]] < 0) t.h.key_slot[cfg->key_body_ids[k]] = k;
    }
    for (int j = 0; j < J; ++j) { t.joint_err_w[j] = cfg->joint_err_w[j]; t.pose_term_dist[j] = cfg->pose_termination_dist[j]; }
    for (int d = 0; d < D; ++d) t.dof_err_w[d] = cfg->dof_err_w[d];
    for (int b = 0; b < B; ++b) t.contact_w[b] = cfg->contact_weights[b];

    StepParams &sp = e->sp;
    memset(&sp, 0, sizeof(sp));
    sp.N = e->N; sp.B = B; sp.J = J; sp.D = D; sp.K = K; sp.S = S; sp.R = R;
    // observation layout (ig_parkour_env.py:842-965)
    sp.global_obs = cfg->global_obs; sp.off_char = cfg->global_root_height_obs ? 1 : 0;
    sp.off_dofvel = sp.off_char + 12 + 6 * J;
    sp.off_key = sp.off_dofvel + D;
    sp.off_tar = sp.off_key + 3 * K;
    sp.tar_w = 3 + 6 + 6 * J + 3 * K;
    e->row_mul = parc_rowmap_mul(B);
    if (!parc_rowmap_mul_ok(B, e->row_mul)) return fail(PARC_ERR_INVALID, "internal: row item multiplier");
    if (!parc_lanetab_fill(t.lane, B, S, D, R, -1, e->row_mul, 0u)) return fail(PARC_ERR_INVALID, "internal: lane table"); // the tile cells follow with the terrain
    sp.lr_identity = 1;
    for (int b = 0; b < B; ++b)
        if (!(cfg->model.local_rotation[b][0] == 0.f && cfg->model.local_rotation[b][1] == 0.f && cfg->model.local_rotation[b][2] == 0.f && cfg->model.local_rotation[b][3] == 1.f)) sp.lr_identity = 0;
    sp.obs_tar = cfg->enable_tar_obs != 0; sp.obs_contact = cfg->use_contact_info != 0;
    sp.off_tarc = sp.off_tar + (sp.obs_tar ? S * sp.tar_w : 0);          // ig_parkour_env.py:927-946: the blocks that exist, in this order
    if (!parc_hrot_fill(t.hrot, B, S, D, K, t.h.key_ids, t.h.key_slot, sp.off_char, sp.off_key, sp.off_tar, sp.tar_w, sp.obs_tar, sp.obs_tar && sp.obs_contact, sp.global_obs, sp.off_tarc))
        return fail(PARC_ERR_INVALID, "internal: heading-pass table");
    sp.off_cc = sp.off_tarc + (sp.obs_tar && sp.obs_contact ? S * B : 0);
    sp.off_hf = sp.off_cc + (sp.obs_contact ? B : 0);
    sp.obs_dim = sp.off_hf + R;
    e->obs_dim = sp.obs_dim;
    for (int q = 0; q < S; ++q) sp.tstep[q] = dt_f * (float)cfg->tar_obs_steps[q];
    sp.dt_f = dt_f; sp.episode_length = cfg->episode_length; sp.min_obs_h = cfg->min_obs_h; sp.max_obs_h = cfg->max_obs_h;
    sp.pose_w = cfg->pose_w; sp.vel_w = cfg->vel_w; sp.root_pos_w = cfg->root_pos_w; sp.root_vel_w = cfg->root_vel_w; sp.key_pos_w = cfg->key_pos_w;
    sp.root_pos_term_sq = (float)((double)cfg->root_pos_termination_dist * (double)cfg->root_pos_termination_dist);
    sp.root_rot_term = cfg->root_rot_termination_angle;
    sp.early_term = cfg->enable_early_termination; sp.pose_term = cfg->pose_termination; sp.track_root = cfg->track_root;
    sp.track_root_h = cfg->track_root_h; sp.tracking = cfg->report_tracking_error; sp.body_pos_from_fk = cfg->body_pos_from_fk;
    sp.fall_mask = cfg->contact_body_mask & ((1u << B) - 1u); sp.term_h = cfg->termination_height;

    DeviceArena &mem = e->mem;
    const long long N = e->N;
    PARC_TRY(mem.alloc(e->d_tab, 1, &t));
    PARC_TRY(mem.alloc_fill(e->d_prep, 16 * N));
    PARC_TRY(mem.alloc(e->d_ray, 2 * R, cfg->ray_points_host));
    PARC_TRY(mem.alloc(e->d_env_off, 3 * N, cfg->env_offsets_host));
    PARC_TRY(mem.alloc_fill(e->d_ema, (N + 1023) / 1024 * 1024));
    PARC_TRY(mem.alloc_fill(e->d_done_list, N));
    PARC_TRY(mem.alloc_fill(e->d_done_key, N));
    PARC_TRY(mem.alloc_fill(e->d_chunk_count, 1024));
    PARC_TRY(mem.alloc_fill(e->d_reset_count, 2));
    PARC_TRY(mem.alloc_fill(e->d_reset_calls, 1));
    PARC_TRY(mem.alloc_fill(e->d_scratch_jr, 4 * J * N));
    { // render geometry: the MJCF collision geoms the scene builder puts into ParcDynamicsParams whether or not the dynamics run
        RenderGeoms rg;
        memset(&rg, 0, sizeof(rg));
        const ParcDynamicsParams &dp = cfg->dynamics;
        for (int g = 0; g < dp.num_geoms && g < PARC_MAX_GEOMS; ++g) {
            if (dp.geom_body[g] < 0 || dp.geom_body[g] >= B || dp.geom_type[g] < PARC_GEOM_BOX || dp.geom_type[g] > PARC_GEOM_CAPSULE) continue;
            const int n = rg.n++;
            rg.body[n] = dp.geom_body[g]; rg.type[n] = dp.geom_type[g];
            for (int c = 0; c < 3; ++c) { rg.p0[n][c] = dp.geom_pos[g][c]; rg.p1[n][c] = dp.geom_pos2[g][c]; rg.size[n][c] = dp.geom_size[g][c]; }
        }
        PARC_TRY(mem.alloc(e->d_rgeom, 1, &rg));
    }
    {
        hipDeviceProp_t prop;
        (void)hipGetDeviceProperties(&prop, cfg->device);
        e->grid_waves = prop.multiProcessorCount * 16; // persistent waves; each strides over envs
        e->num_cus = prop.multiProcessorCount;
    }
    if (cfg->enable_dynamics) PARC_TRY(parc_dyn_create(cfg, e->N, e->num_cus, &e->dyn));
    e->force_ema_leader = !dev_opt(cfg, "ema_leader").empty();
    e->force_two_launch_curriculum = !dev_opt(cfg, "curriculum_two_launches").empty();
    if (hipHostMalloc((void **)&e->h_health, 2 * sizeof(unsigned int), hipHostMallocMapped) == hipSuccess) {
        e->h_health[0] = 0u; e->h_health[1] = 0u;
        if (hipHostGetDevicePointer((void **)&e->d_health, e->h_health, 0) != hipSuccess) e->d_health = nullptr;
    }
    if (e->dyn && e->d_health) {
        e->health.words = e->d_health;
        PARC_TRY(parc_dyn_counters(&e->health.from));
    }
    PARC_TRY(e->ev.create());
    sp.tables = e->d_tab; sp.ray_points = e->d_ray; sp.env_offsets = e->d_env_off;
    sp.ema_code = e->d_ema; sp.prep = e->d_prep;
#ifdef PARC_STAMPS
    PARC_TRY(mem.alloc(sp.stamp_out, 8 * N));
#endif
    e->nchunks = (e->N + 1023) / 1024;

    *out = e.release();
    return PARC_OK;
}

extern "C" void parc_env_destroy(ParcEnv *e) { delete e; }

extern "C" int parc_env_obs_dim(const ParcEnv *e) { return e ? e->obs_dim : PARC_ERR_INVALID; }

// The two loads build the new state in locals and swap it into the handle as their last step: a call that returns non-zero has
// changed nothing (the local arenas release what it allocated), a call that succeeds leaves the old state to the local arena.
extern "C" int parc_env_load_motions(ParcEnv *e, const ParcMotionClips *c) {
    if (!e || !c || c->num_motions < 1) return fail(PARC_ERR_INVALID, "bad motion clips");
    const int M = c->num_motions, B = e->B, J = e->J;
    std::vector<MotionMeta> meta;
    std::vector<float> weights;
    std::vector<int> frame_motion;
    if (const char *msg = parc_motion_table(M, c->num_frames_host, c->fps_host, c->loop_modes_host, c->weights_host, c->root_pos_host, meta, weights, frame_motion))
        return fail(PARC_ERR_INVALID, msg);
    const long long F = (long long)frame_motion.size();
    HIPCHK(hipSetDevice(e->cfg.device));
    DeviceArena set, tmp; // the new motion set / the inputs of k_motion_prep
    float4 *d_records;
    MotionMeta *d_meta;
    float *d_weights, *d_fail, *d_cdf;
    int *d_motion_done;
    const std::vector<float> ones((size_t)M, 1.0f); // dm_env.py:87
    PARC_TRY(set.alloc(d_records, REC_F4 * F));
    PARC_TRY(set.alloc(d_meta, M, meta.data()));
    PARC_TRY(set.alloc(d_weights, M, weights.data()));
    PARC_TRY(set.alloc(d_fail, M, ones.data()));
    PARC_TRY(set.alloc(d_cdf, M));
    PARC_TRY(set.alloc_fill(d_motion_done, M, 0x7f)); // 0x7f7f7f7f: larger than any list index (k_ema_first takes the minimum)
    PrepParams pp;
    pp.F = (int)F; pp.B = B; pp.J = J; pp.D = e->D; pp.contacts = nullptr;
    pp.meta = d_meta; pp.tables = e->d_tab; pp.records = d_records;
    PARC_TRY(tmp.alloc(pp.root_pos, 3 * F, c->root_pos_host));
    PARC_TRY(tmp.alloc(pp.root_rot, 4 * F, c->root_rot_host));
    PARC_TRY(tmp.alloc(pp.joint_rot, 4 * J * F, c->joint_rot_host));
    PARC_TRY(tmp.alloc(pp.frame_motion, F, frame_motion.data()));
    if (c->contacts_host) PARC_TRY(tmp.alloc(pp.contacts, B * F, c->contacts_host));
    hipLaunchKernelGGL(k_motion_prep, dim3((unsigned)((F + 127) / 128)), dim3(128), 0, 0, pp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());

    e->motions.swap(set);
    e->h_meta.swap(meta); e->h_weights.swap(weights);
    e->d_records = d_records; e->d_meta = d_meta; e->d_weights = d_weights; e->d_fail = d_fail; e->d_cdf = d_cdf; e->d_motion_done = d_motion_done;
    if (M != e->M) e->have_terrain = false; // motion_offsets has one row per motion of the old set: parc_env_load_terrain again
    e->M = M; e->F = F; e->have_motions = true;
    e->sp.M = M; e->sp.records = d_records; e->sp.meta = d_meta;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_load_terrain(ParcEnv *e, const float *hf, int32_t X, int32_t Y, float min_x, float min_y, float dx, float dy,
                                     const float *motion_offsets, int32_t M, int32_t T) {
    if (!e || !hf || !motion_offsets || X < 1 || Y < 1 || T < 1 || !(dx > 0.f) || !(dy > 0.f)) return fail(PARC_ERR_INVALID, "bad terrain");
    if (!e->have_motions || M != e->M) return fail(PARC_ERR_STATE, "load_motions first; motion_offsets must have one row per motion");
    HIPCHK(hipSetDevice(e->cfg.device));
    // terrain tile radius: farthest ray sample in cells, +1 for the two independent roundings
    std::vector<float> ray(2 * (size_t)e->R);
    HIPCHK(hipMemcpy(ray.data(), e->d_ray, sizeof(float) * 2 * e->R, hipMemcpyDeviceToHost));
    float rmax = 0.f;
    for (int r = 0; r < e->R; ++r) rmax = fmaxf(rmax, sqrtf(ray[2 * r] * ray[2 * r] + ray[2 * r + 1] * ray[2 * r + 1]));
    int tr = (int)ceilf(rmax / fminf(dx, dy) + 0.01f); // max |round(a+d)-round(a)| = ceil(|d|)
    if ((2 * tr + 1) * (2 * tr + 1) > TILE_MAX_CELLS) tr = -1; // fan too wide for the LDS tile: direct gathers
    unsigned tile_mul = 0; // idx / (2 tr + 1) == (idx * tile_mul) >> 16, which only the fill of the tile cells needs: unused without a tile
    if (tr >= 0) { // magic multiplier for idx / TW, verified for every cell of the tile
        const unsigned TW = 2 * tr + 1;
        tile_mul = (65536u + TW - 1) / TW;
        for (unsigned idx = 0; idx < TW * TW; ++idx)
            if (((idx * tile_mul) >> 16) != idx / TW) return fail(PARC_ERR_INVALID, "internal: tile index multiplier");
    }
    ParcLaneEntry lanes[64]; // the lane table that holds the tile cells (parc_lanetab.hpp)
    if (!parc_lanetab_fill(lanes, e->B, e->S, e->D, e->R, tr, e->row_mul, tile_mul)) return fail(PARC_ERR_INVALID, "internal: lane table");
    const size_t cells = (size_t)X * Y;
    float hf_max = hf[0], hf_min = hf[0];
    for (size_t q = 1; q < cells; ++q) { hf_max = fmaxf(hf_max, hf[q]); hf_min = fminf(hf_min, hf[q]); }
    DeviceArena ter;
    float *d_hf, *d_motion_off;
    PARC_TRY(ter.alloc(d_hf, (long long)cells, hf));
    PARC_TRY(ter.alloc(d_motion_off, 2LL * M * T, motion_offsets));
    HIPCHK(hipMemcpy(e->d_tab->lane, lanes, sizeof(lanes), hipMemcpyHostToDevice)); // the last step that can fail

    e->terrain.swap(ter);
    e->d_hf = d_hf; e->d_motion_off = d_motion_off;
    StepParams &sp = e->sp;
    sp.hf = d_hf; sp.X = X; sp.Y = Y; sp.min_x = min_x; sp.min_y = min_y; sp.dx = dx; sp.dy = dy; sp.T = T;
    sp.rdx = (float)(1.0L / (long double)dx); sp.rdy = (float)(1.0L / (long double)dy);
    sp.motion_offsets = d_motion_off;
    e->T = T;
    e->hf_max = hf_max; e->hf_min = hf_min;
    sp.tile_r = tr;
    memcpy(e->h_tab.lane, lanes, sizeof(lanes));
    const int stage_pad = (sp.off_tarc + 3) & ~3;
    e->lds_bytes = sizeof(float) * (size_t)stage_pad + (e->cfg.report_tracking_error ? 2 * 16 * sizeof(float4) : 0); // per wave of k_env_post
    sp.lds_wave_floats = (int)(e->lds_bytes / sizeof(float));
    e->have_terrain = true;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_bind_buffers(ParcEnv *e, const ParcEnvBuffers *b) {
    if (!e || !b) return fail(PARC_ERR_INVALID, "null argument");
    const void *req[] = {b->char_root_pos, b->char_root_rot, b->char_root_vel, b->char_root_ang_vel, b->char_dof_pos, b->char_dof_vel,
                         b->contact_forces, b->motion_ids, b->terrain_ids, b->time_offsets, b->timestep, b->obs, b->reward, b->done};
    for (const void *p : req) if (!p) return fail(PARC_ERR_INVALID, "a required buffer is NULL");
    if (!e->cfg.body_pos_from_fk && !b->char_body_pos) return fail(PARC_ERR_INVALID, "char_body_pos is required when body_pos_from_fk == 0");
    if (((uintptr_t)b->obs & 15) != 0) return fail(PARC_ERR_INVALID, "obs must be 16-byte aligned");
    if ((b->ref_root_rot && ((uintptr_t)b->ref_root_rot & 15)) || (b->ref_joint_rot && ((uintptr_t)b->ref_joint_rot & 15)) ||
        ((uintptr_t)b->char_root_rot & 15))
        return fail(PARC_ERR_INVALID, "quaternion buffers must be 16-byte aligned");
    e->sp.buf = *b;
    e->bound = true;
    e->graph_dirty = true;
    return PARC_OK;
}

static int check_ready(ParcEnv *e) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    if (!e->bound || !e->have_motions || !e->have_terrain) return fail(PARC_ERR_STATE, "bind_buffers, load_motions and load_terrain must precede this call");
    return PARC_OK;
}

static int launch_dynamics(ParcEnv *e, const float *action_dev, hipStream_t st) {
    if (!e->dyn) return PARC_OK;
    const ParcDynTerrain T = {e->d_hf, e->sp.X, e->sp.Y, e->sp.min_x, e->sp.min_y, e->sp.dx, e->sp.dy};
    return parc_dyn_launch(e->dyn, T, e->sp.buf, action_dev, e->d_env_off, e->d_prep, st);
}

// Which of the three curriculum paths a handle takes, with the name parc_env_describe prints for it.
enum CurriculumPath { CURRICULUM_ONE_LAUNCH, CURRICULUM_BLOCK_PER_MOTION, CURRICULUM_LEADER };
static const char *const CURRICULUM_PATH_NAME[] = {"k_curriculum_small", "k_done_scatter+k_fail_rate_ema", "k_done_scatter+k_ema_first+k_ema_leader"};
static CurriculumPath curriculum_path(const ParcEnv *e) {
    if (e->M > 64 || e->force_ema_leader) return CURRICULUM_LEADER; // large libraries: one wave per list entry, the leaders walk the list
    if (e->N <= CURRICULUM_ONE_LAUNCH_MAX && (e->N & 7) == 0 && !e->force_two_launch_curriculum) return CURRICULUM_ONE_LAUNCH;
    return CURRICULUM_BLOCK_PER_MOTION;
}

static int launch_curriculum(ParcEnv *e, hipStream_t st) {
    e->done_list_fresh = true;
    const CurriculumPath path = curriculum_path(e);
    if (path == CURRICULUM_ONE_LAUNCH) {
        hipLaunchKernelGGL(k_curriculum_small, dim3(e->nchunks + e->M), dim3(1024), 0, st, e->d_ema, e->sp.buf.motion_ids, e->N, e->d_done_list,
                           e->d_done_key, e->d_reset_count, e->sp.never_done, e->nchunks, e->d_fail, e->M, e->cfg.fail_rate_ema_weight, e->health);
        HIPCHK(hipGetLastError());
        return PARC_OK;
    }
    hipLaunchKernelGGL(k_done_scatter, dim3(e->nchunks), dim3(1024), 0, st, e->d_ema, e->sp.buf.motion_ids, e->N, e->d_done_list,
                       e->d_done_key, e->d_reset_count, e->sp.never_done, e->health);
    if (path == CURRICULUM_BLOCK_PER_MOTION) {
        hipLaunchKernelGGL(k_fail_rate_ema, dim3(e->M), dim3(1024), 0, st, e->d_done_key, e->d_reset_count, e->d_fail, e->M,
                           e->cfg.fail_rate_ema_weight);
    } else { // d_motion_done doubles as the per-motion "first list entry" slot (INT_MAX between steps)
        hipLaunchKernelGGL(k_ema_first, dim3((e->N + 255) / 256), dim3(256), 0, st, e->d_done_key, e->d_reset_count, e->d_motion_done);
        hipLaunchKernelGGL(k_ema_leader, dim3((e->N + 3) / 4), dim3(256), 0, st, e->d_done_key, e->d_reset_count, e->d_motion_done, e->d_fail,
                           e->cfg.fail_rate_ema_weight);
    }
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

// an observation layout other than the default one: the OBSVAR instantiations of k_env_post decide it at run time
static bool obs_variant(const ParcEnvConfig &c) { return c.global_obs || c.global_root_height_obs || !c.use_contact_info || !c.enable_tar_obs; }

static bool wants_mirror(const ParcEnvBuffers &b) {
    return b.ref_root_pos || b.ref_root_rot || b.ref_root_vel || b.ref_root_ang_vel || b.ref_joint_rot || b.ref_dof_pos || b.ref_dof_vel ||
           b.ref_body_pos || b.ref_contacts || b.ray_hfs || b.tracking_error;
}

// The instantiation of k_env_post a launch in `mode` (MODE_STEP / MODE_OBS) takes, and the name parc_env_post_kernel prints for it.
typedef void (*PostKernelFn)(const StepParams, const int64_t *, const int *, const int *, int, unsigned long long *);
struct PostKernel { PostKernelFn fn; const char *name; };
static PostKernel post_kernel(const ParcEnv *e, int mode) {
    const bool step = mode == MODE_STEP;
    const bool local = step && !e->sp.track_root; // track_root: false -- the reward in the characters' heading frames
    if (obs_variant(e->cfg)) // a non-default observation layout -- instantiated for the general (MIRROR) form only
        return {local ? k_env_post<MODE_STEP, true, true, true> : step ? k_env_post<MODE_STEP, true, false, true> : k_env_post<MODE_OBS, true, false, true>,
                "k_env_post<MODE,true>"};
    if (wants_mirror(e->sp.buf))
        return {local ? k_env_post<MODE_STEP, true, true> : step ? k_env_post<MODE_STEP, true> : k_env_post<MODE_OBS, true>, "k_env_post<MODE,true>"};
    return {local ? k_env_post<MODE_STEP, false, true> : step ? k_env_post<MODE_STEP, false> : k_env_post<MODE_OBS, false>, "k_env_post<MODE,false>"};
}

static int launch_post(ParcEnv *e, int mode, const int64_t *ids, int count, hipStream_t st, const int *ids32 = nullptr,
                       const int *count_dev = nullptr, bool prep_done = false, unsigned long long *bump = nullptr) {
    if (count <= 0) return PARC_OK;
    const int grid = (count + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK;
    const size_t lds = e->lds_bytes * ENVS_PER_BLOCK;
    if (mode == MODE_STEP && e->dyn && parc_dyn_writes_prep(e->dyn)) prep_done = true; // k_dynamics_wave wrote the prep records with the state
    if (!prep_done) hipLaunchKernelGGL(k_env_prep, dim3((count + 3) / 4), dim3(64), 0, st, e->sp, ids, ids32, count_dev, count);
    hipLaunchKernelGGL(post_kernel(e, mode).fn, dim3(grid), dim3(64 * ENVS_PER_BLOCK), lds, st, e->sp, ids, ids32, count_dev, count, bump);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

// One control step on `st`: dynamics -> observation / reward / done -> curriculum.  `ev` (optional): four events, recorded in front of,
// between and behind the three.
static int step_sequence(ParcEnv *e, const float *action_dev, hipStream_t st, const hipEvent_t *ev) {
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    PARC_TRY(launch_dynamics(e, action_dev, st));
    if (ev) HIPCHK(hipEventRecord(ev[1], st));
    PARC_TRY(launch_post(e, MODE_STEP, nullptr, e->N, st));
    if (ev) HIPCHK(hipEventRecord(ev[2], st));
    PARC_TRY(launch_curriculum(e, st));
    if (ev) HIPCHK(hipEventRecord(ev[3], st));
    return PARC_OK;
}

extern "C" int parc_env_step(ParcEnv *e, const float *action_dev, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    const hipEvent_t *tv = nullptr;
    if (e->timing) { // no host synchronisation: events come from a growing pool and are read back by parc_env_get_kernel_timing
        if (e->tev_used + 4 > e->tev.size()) {
            const size_t old = e->tev.size();
            e->tev.resize(old + 1024, nullptr);
            for (size_t i = old; i < e->tev.size(); ++i) HIPCHK(hipEventCreate(&e->tev[i]));
        }
        tv = &e->tev[e->tev_used];
        e->tev_used += 4;
    }
    return step_sequence(e, action_dev, (hipStream_t)stream, tv);
}

extern "C" int parc_env_get_buffers(ParcEnv *e, ParcEnvBuffers *out) {
    if (!e || !out) return fail(PARC_ERR_INVALID, "null argument");
    if (!e->bound) return fail(PARC_ERR_STATE, "bind_buffers first");
    *out = e->sp.buf;
    return PARC_OK;
}

extern "C" int parc_env_set_episode_length(ParcEnv *e, float seconds) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    if (!(seconds > 0.f)) return fail(PARC_ERR_INVALID, "episode length must be positive");
    e->sp.episode_length = seconds;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_record_bind(ParcEnv *e, float *frames_dev, float *obs_dev, int32_t cap, int32_t *count_dev, uint8_t *writing_dev,
                                    int32_t *n_writing_dev, int32_t record_ref) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    if (!frames_dev) { e->rec_frames = nullptr; e->rec_cap = 0; return PARC_OK; } // unbind
    if (cap < 1 || !count_dev || !writing_dev || !n_writing_dev) return fail(PARC_ERR_INVALID, "recorder buffers are incomplete");
    if (!e->bound) return fail(PARC_ERR_STATE, "bind_buffers must precede record_bind");
    if (record_ref && (!e->sp.buf.ref_root_pos || !e->sp.buf.ref_root_rot || !e->sp.buf.ref_joint_rot || !e->sp.buf.ref_contacts))
        return fail(PARC_ERR_STATE, "record_ref needs the ref_* mirrors to be bound");
    e->rec_frames = frames_dev; e->rec_obs = obs_dev; e->rec_cap = cap; e->rec_count = count_dev; e->rec_writing = writing_dev;
    e->rec_nwriting = n_writing_dev; e->rec_ref = record_ref ? 1 : 0;
    return PARC_OK;
}

extern "C" int parc_env_record_frame(ParcEnv *e, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (!e->rec_frames) return fail(PARC_ERR_STATE, "no recorder buffers bound");
    hipLaunchKernelGGL(k_record, dim3(e->N), dim3(128), 0, (hipStream_t)stream, (const DevTables *)e->d_tab, e->sp.buf, e->N, e->B, e->D,
                       e->obs_dim, e->rec_frames, e->rec_obs, e->rec_cap, e->rec_count, e->rec_writing, e->rec_nwriting, e->rec_ref);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_env_set_kernel_timing(ParcEnv *e, int32_t enable) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    e->timing = enable != 0;
    e->tev_used = 0;
    return PARC_OK;
}

// Timed step i (step_sequence with the events of parc_env_step): the time of the dynamics kernel, of the observation kernels and of the
// curriculum launches that close the step.
static int timed_step_ms(ParcEnv *e, size_t i, float &dynamics_ms, float &obs_ms, float &curriculum_ms) {
    const hipEvent_t *tv = &e->tev[4 * i];
    HIPCHK(hipEventSynchronize(tv[3]));
    HIPCHK(hipEventElapsedTime(&dynamics_ms, tv[0], tv[1]));
    HIPCHK(hipEventElapsedTime(&obs_ms, tv[1], tv[2]));
    HIPCHK(hipEventElapsedTime(&curriculum_ms, tv[2], tv[3]));
    return PARC_OK;
}

// Per-step samples of the same events (call BEFORE parc_env_get_kernel_timing, which clears them): up to `cap` steps, dynamics kernel /
// observation kernel / the curriculum launches that close the step.  Returns the number of steps recorded in *steps.
extern "C" int parc_env_get_kernel_timing_samples(ParcEnv *e, float *dynamics_ms, float *obs_ms, float *curriculum_ms, int32_t cap, int32_t *steps) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    const size_t n = e->tev_used / 4;
    for (size_t i = 0; i < n && (int32_t)i < cap; ++i) {
        float a = 0.f, b = 0.f, c = 0.f;
        PARC_TRY(timed_step_ms(e, i, a, b, c));
        if (dynamics_ms) dynamics_ms[i] = a;
        if (obs_ms) obs_ms[i] = b;
        if (curriculum_ms) curriculum_ms[i] = c;
    }
    if (steps) *steps = (int32_t)n;
    return PARC_OK;
}

extern "C" int parc_env_get_kernel_timing(ParcEnv *e, double *dynamics_ms_avg, double *obs_ms_avg, int32_t *steps) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    const size_t n = e->tev_used / 4;
    double dyn = 0.0, post = 0.0;
    for (size_t i = 0; i < n; ++i) {
        float a = 0.f, b = 0.f, c = 0.f;
        PARC_TRY(timed_step_ms(e, i, a, b, c));
        dyn += a; post += b;
    }
    if (dynamics_ms_avg) *dynamics_ms_avg = n ? dyn / (double)n : 0.0;
    if (obs_ms_avg) *obs_ms_avg = n ? post / (double)n : 0.0;
    if (steps) *steps = (int32_t)n;
    e->tev_used = 0;
    return PARC_OK;
}

extern "C" int parc_env_compute_obs(ParcEnv *e, const int64_t *ids, int32_t k, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (k == 0) return PARC_OK;
    if (k > 0 && !ids) return fail(PARC_ERR_INVALID, "env_ids is NULL");
    return launch_post(e, MODE_OBS, k < 0 ? nullptr : ids, k < 0 ? e->N : k, (hipStream_t)stream);
}

// A reset of the n envs of a list (dm_env.py:567-592) and the observation pass over them.  With mids (and tids, t0, noise) the caller
// has drawn the samples, one per list entry; without, it is a sampling reset (dm_env.py:470-504): [k_build_cdf for libraries of more than
// CDF_LOCAL_MAX motions,] k_reset_with drawing motion / terrain / start time / xy noise per env, and the observation pass bumps the
// Philox call index.
static int launch_reset(ParcEnv *e, const int64_t *ids, const int *ids32, const int *count_dev, int n, const int *mids, const int *tids,
                        const float *t0, const float *noise, hipStream_t st) {
    const bool sampling = !mids;
    ResetParams rp;
    rp.B = e->B; rp.J = e->J; rp.D = e->D; rp.T = e->T; rp.N = e->N;
    rp.records = e->d_records; rp.meta = e->d_meta; rp.motion_offsets = e->d_motion_off; rp.env_offsets = e->d_env_off;
    rp.tables = e->d_tab; rp.scratch_jr = e->d_scratch_jr; rp.prep = e->d_prep; rp.buf = e->sp.buf;
    SampleParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.enabled = sampling ? 1 : 0;
    sp.M = e->M; sp.T = e->T; sp.rand_reset = e->cfg.rand_reset; sp.demo_mode = e->cfg.demo_mode;
    sp.min_w = e->cfg.min_motion_weight; sp.noise_scale = e->cfg.rand_root_pos_offset_scale;
    sp.cdf_global = e->d_cdf; sp.fail_rates = e->d_fail; sp.motion_weights = e->d_weights; sp.start_frac = e->d_start_frac;
    sp.seed = (unsigned long long)e->cfg.seed; sp.call_dev = e->d_reset_calls;
    if (sampling && e->M > CDF_LOCAL_MAX)
        hipLaunchKernelGGL(k_build_cdf, dim3(1), dim3(1024), 0, st, e->d_fail, e->d_weights, e->cfg.min_motion_weight, e->M, e->d_cdf);
    hipLaunchKernelGGL(k_reset_with, dim3((n + 3) / 4), dim3(64), 0, st, rp, ids, ids32, count_dev, n, mids, tids, t0, noise, sp);
    HIPCHK(hipGetLastError());
    return launch_post(e, MODE_OBS, ids, n, st, ids32, count_dev, /*prep_done=*/true, sampling ? e->d_reset_calls : nullptr);
}

extern "C" int parc_env_reset_with(ParcEnv *e, const int64_t *ids, int32_t k, const int32_t *mids, const int32_t *tids, const float *t0,
                                   const float *noise, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (k == 0) return PARC_OK;
    if (k > e->N) return fail(PARC_ERR_INVALID, "k > num_envs");
    if (!mids || !tids || !t0 || !noise || (k > 0 && !ids)) return fail(PARC_ERR_INVALID, "null sample array");
    return launch_reset(e, k < 0 ? nullptr : ids, nullptr, nullptr, k < 0 ? e->N : k, mids, tids, t0, noise, (hipStream_t)stream);
}

extern "C" int parc_env_reset(ParcEnv *e, const int64_t *ids, int32_t k, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (k == 0) return PARC_OK;
    if (k > e->N) return fail(PARC_ERR_INVALID, "k > num_envs");
    if (k > 0 && !ids) return fail(PARC_ERR_INVALID, "env_ids is NULL");
    return launch_reset(e, k < 0 ? nullptr : ids, nullptr, nullptr, k < 0 ? e->N : k, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

// Reset every env whose done flag was raised by the last step (base_agent.py:366-370) without the
// nonzero()/host round trip: the step kernel's compacted done list and its device-side count drive the launch.
// The list is consumed by the call: a second call before the next step resets nobody.
extern "C" int parc_env_reset_done(ParcEnv *e, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (!e->done_list_fresh) return PARC_OK;
    e->done_list_fresh = false;
    return launch_reset(e, nullptr, e->d_done_list, e->d_reset_count + 1, e->N, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

// ---- whole control step as one hipGraph launch ----------------------------------------------------------------------
// step + reset_done are ~10 dependent launches; at a few thousand envs the host-side launch cost exceeds the kernels.
// The sequence is captured once on a private stream and replayed with one hipGraphLaunch.  Everything a kernel argument
// bakes in is either fixed per handle (buffers, tables), re-captured when it changes (graph_dirty), or read from device
// memory (done count, reset-call index, the bound action buffer).
extern "C" int parc_env_bind_action(ParcEnv *e, const float *action_dev) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    e->action_bound = action_dev;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_step_reset_graph(ParcEnv *e, void *stream) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (e->cfg.enable_dynamics && !e->action_bound) return fail(PARC_ERR_STATE, "parc_env_bind_action must precede the graph step when dynamics is on");
    if (e->graph_dirty || !e->graph_exec) {
        if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
        hipStream_t cs = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        hipError_t err = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (err == hipSuccess) {
            const bool timing = e->timing;
            e->timing = false; // events are not captured
            rc = parc_env_step(e, e->action_bound, cs);
            if (!rc) rc = parc_env_reset_done(e, cs);
            e->timing = timing;
            err = hipStreamEndCapture(cs, &graph);
        }
        if (err == hipSuccess && !rc) err = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipStreamDestroy(cs);
        if (rc) return rc;
        if (err != hipSuccess) { e->graph_exec = nullptr; return fail(PARC_ERR_HIP, std::string("graph capture failed: ") + hipGetErrorString(err)); }
        e->graph_dirty = false;
    }
    HIPCHK(hipGraphLaunch(e->graph_exec, (hipStream_t)stream));
    e->done_list_fresh = false; // the graph holds step + reset_done
    return PARC_OK;
}

extern "C" int parc_env_get_fail_rates(ParcEnv *e, float *out, int32_t M) {
    if (!e || !out || !e->have_motions || M != e->M) return fail(PARC_ERR_INVALID, "bad fail-rate query");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, e->d_fail, sizeof(float) * M, hipMemcpyDeviceToHost));
    return PARC_OK;
}

extern "C" int parc_env_set_fail_rates(ParcEnv *e, const float *in, int32_t M) {
    if (!e || !in || !e->have_motions || M != e->M) return fail(PARC_ERR_INVALID, "bad fail-rate update");
    HIPCHK(hipSetDevice(e->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(e->d_fail, in, sizeof(float) * M, hipMemcpyHostToDevice));
    return PARC_OK;
}

extern "C" int parc_env_get_motion_info(ParcEnv *e, float *lengths, float *weights, int32_t M) {
    if (!e || !e->have_motions || M != e->M) return fail(PARC_ERR_INVALID, "bad motion-info query");
    for (int m = 0; m < M; ++m) {
        if (lengths) lengths[m] = e->h_meta[m].length;
        if (weights) weights[m] = e->h_weights[m];
    }
    return PARC_OK;
}

extern "C" int parc_env_set_never_done(ParcEnv *e, int32_t never_done) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    e->sp.never_done = never_done != 0;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_set_rand_reset(ParcEnv *e, int32_t rand_reset, int32_t demo_mode, float scale) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    e->cfg.rand_reset = rand_reset; e->cfg.demo_mode = demo_mode; e->cfg.rand_root_pos_offset_scale = scale;
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_env_set_start_time_fraction(ParcEnv *e, const float *frac_dev) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    e->d_start_frac = const_cast<float *>(frac_dev);
    e->graph_dirty = true;
    return PARC_OK;
}

extern "C" int parc_dof_to_rot(ParcEnv *e, const float *dof, float *jr, int32_t n, void *stream) {
    if (!e || !dof || !jr || n < 0) return fail(PARC_ERR_INVALID, "bad argument");
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(k_dof_to_rot, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e->d_tab, dof, jr, n, e->B, e->D);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_rot_to_dof(ParcEnv *e, const float *jr, float *dof, int32_t n, void *stream) {
    if (!e || !dof || !jr || n < 0) return fail(PARC_ERR_INVALID, "bad argument");
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(k_rot_to_dof, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e->d_tab, jr, dof, n, e->B, e->D);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_forward_kinematics(ParcEnv *e, const float *rp, const float *rr, const float *jr, float *bp, float *br, int32_t n,
                                       void *stream) {
    if (!e || !rp || !rr || !jr || !bp || n < 0) return fail(PARC_ERR_INVALID, "bad argument");
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(k_fk, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e->d_tab, rp, rr, jr, bp, br, n, e->B);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_calc_motion_frame(ParcEnv *e, const int32_t *ids, const float *times, int32_t n, float *rp, float *rr, float *rv,
                                      float *rav, float *jr, float *dv, float *ct, void *stream) {
    if (!e || !e->have_motions) return fail(PARC_ERR_STATE, "load_motions first");
    if (!ids || !times || !rp || !rr || !jr || n < 0) return fail(PARC_ERR_INVALID, "bad argument");
    if (n == 0) return PARC_OK;
    FrameOut F;
    F.root_pos = rp; F.root_rot = rr; F.root_vel = rv; F.root_ang_vel = rav; F.joint_rot = jr; F.dof_vel = dv; F.contacts = ct;
    hipLaunchKernelGGL(k_calc_motion_frame, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, e->d_records, e->d_meta, ids, times, n,
                       e->B, e->J, e->D, F);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_test_quat_op(int32_t op, const float *a, const float *b, const float *t, int32_t n, float *out, void *stream) {
    if (!a || !out || n < 0 || op < 0 || op > PARC_QOP_SLERP_RR) return fail(PARC_ERR_INVALID, "bad argument");
    if ((op == PARC_QOP_MUL || op == PARC_QOP_ROTATE || op == PARC_QOP_DIFF_ANGLE || op == PARC_QOP_SLERP || op == PARC_QOP_SLERP_RR || op == PARC_QOP_DIFF) && !b)
        return fail(PARC_ERR_INVALID, "this op needs a second operand");
    if ((op == PARC_QOP_AA_TO_QUAT || op == PARC_QOP_SLERP || op == PARC_QOP_SLERP_RR || op == PARC_QOP_ROTATE_2D) && !t) return fail(PARC_ERR_INVALID, "this op needs the scalar operand");
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(k_test_quat_op, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, (int)op, a, b, t, (int)n, out);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

extern "C" int parc_env_get_frame_vel_tables(ParcEnv *e, float *root_vel, float *root_ang_vel, float *dof_vel) {
    if (!e || !e->have_motions) return fail(PARC_ERR_STATE, "load_motions first");
    HIPCHK(hipSetDevice(e->cfg.device));
    std::vector<float> rec((size_t)e->F * 128);
    HIPCHK(hipMemcpy(rec.data(), e->d_records, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t f = 0; f < e->F; ++f) {
        const float *v = rec.data() + (size_t)f * 128 + 4 * REC_Q_VEL;
        if (root_vel) for (int c = 0; c < 3; ++c) root_vel[3 * f + c] = v[c];
        if (root_ang_vel) for (int c = 0; c < 3; ++c) root_ang_vel[3 * f + c] = v[4 + c];
        if (dof_vel) for (int d = 0; d < e->D; ++d) dof_vel[(size_t)f * e->D + d] = v[8 + d];
    }
    return PARC_OK;
}

extern "C" const unsigned int *parc_env_health_words(ParcEnv *e) { return (e && e->d_health) ? e->h_health : nullptr; }

extern "C" const char *parc_env_describe(ParcEnv *e) {
    if (!e) return "";
    char b[1024];
    std::string d = e->dyn ? parc_dyn_describe(e->dyn) : "dynamics_kernel=none;";
    snprintf(b, sizeof(b), "curriculum=%s;post_kernel=%s;dev_options=%s", CURRICULUM_PATH_NAME[curriculum_path(e)],
             e->bound ? parc_env_post_kernel(e) : "unbound", e->dev_options_s.empty() ? "none" : e->dev_options_s.c_str());
    d += b;
    e->describe_s = d;
    return e->describe_s.c_str();
}

// The process-wide counters of k_dynamics_wave on the env's device (parc_dynamics_host.hpp): both must stay 0.
extern "C" int parc_env_dynamics_timeouts(ParcEnv *e) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    return parc_dyn_read_counter(false);
}

extern "C" int parc_env_dynamics_manifold_drops(ParcEnv *e) {
    if (!e) return fail(PARC_ERR_INVALID, "null env");
    HIPCHK(hipSetDevice(e->cfg.device));
    return parc_dyn_read_counter(true);
}

extern "C" float parc_env_last_dynamics_ms(ParcEnv *e) { return e ? e->last_dyn_ms : 0.f; }

extern "C" const char *parc_env_dynamics_kernel(ParcEnv *e) {
    return (e && e->dyn) ? parc_dyn_kernel_name(e->dyn) : "";
}

extern "C" const char *parc_env_post_kernel(ParcEnv *e) {
    if (!e || !e->bound) return "";
    return post_kernel(e, MODE_STEP).name;
}

// What both render entry points do before they touch the device: the checks of ParcRenderParams and of the handle, in one order, and the
// RenderArgs.  `who` ("render" / "render_scene") prefixes the messages, `the_ref` is their name for what draw_ref draws, and `list_check`
// is the entry point's own check of its env list, at its place among the others.
template <class ListCheck>
static int render_args(ParcEnv *e, const ParcRenderParams *p, const std::string &who, const char *the_ref, ListCheck list_check,
                       const int64_t *env_ids_dev, uint8_t *rgba_dev, float *depth_dev, uint8_t *id_dev, RenderArgs &A) {
    if (!p) return fail(PARC_ERR_INVALID, "null ParcRenderParams");
    if (p->struct_size != sizeof(ParcRenderParams)) return fail(PARC_ERR_INVALID, "ParcRenderParams ABI mismatch (struct_size)");
    if (int rc = check_ready(e)) return rc;
    if (p->width < 8 || p->width > 4096 || p->height < 8 || p->height > 4096) return fail(PARC_ERR_INVALID, who + ": width and height must be in [8, 4096]");
    if (int rc = list_check()) return rc;
    if (p->camera_mode != PARC_CAMERA_TRACK && p->camera_mode != PARC_CAMERA_STILL) return fail(PARC_ERR_INVALID, who + ": unknown camera_mode");
    if (!(p->fov_y > 0.f && p->fov_y < 3.1f)) return fail(PARC_ERR_INVALID, who + ": fov_y must be in (0, 3.1) radians");
    const ParcEnvBuffers &b = e->sp.buf;
    if (p->draw_ref && (!b.ref_root_pos || !b.ref_root_rot || !b.ref_joint_rot || (p->debug_visuals && !b.ref_contacts)))
        return fail(PARC_ERR_STATE, who + ": " + the_ref + " the ref_* mirrors bound (ref_root_pos, ref_root_rot, ref_joint_rot, ref_contacts)");
    const float sl = sqrtf(p->sun_dir[0] * p->sun_dir[0] + p->sun_dir[1] * p->sun_dir[1] + p->sun_dir[2] * p->sun_dir[2]);
    if (!(sl > 1e-6f)) return fail(PARC_ERR_INVALID, who + ": sun_dir must be non-zero");
    if (p->camera_mode == PARC_CAMERA_TRACK) {
        const float *o = p->offset;
        if (!(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] > 1e-12f)) return fail(PARC_ERR_INVALID, who + ": the track offset must be non-zero");
    } else {
        const float dx = p->eye[0] - p->target[0], dy = p->eye[1] - p->target[1], dz = p->eye[2] - p->target[2];
        if (!(dx * dx + dy * dy + dz * dz > 1e-12f)) return fail(PARC_ERR_INVALID, who + ": eye and target coincide");
    }
    memset(&A, 0, sizeof(A));
    A.W = p->width; A.H = p->height; A.N = e->N; A.B = e->B; A.D = e->D;
    A.cam_mode = p->camera_mode; A.draw_ref = p->draw_ref ? 1 : 0; A.shadows = p->shadows ? 1 : 0; A.debug = p->debug_visuals ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        A.off[c] = p->offset[c]; A.eye[c] = p->eye[c]; A.tgt[c] = p->target[c]; A.ref_off[c] = p->ref_offset[c]; A.sun[c] = p->sun_dir[c] / sl;
    }
    A.tan_half = tanf(0.5f * p->fov_y); A.aspect = (float)p->width / (float)p->height;
    A.env_ids = env_ids_dev;
    A.root_pos = b.char_root_pos; A.root_rot = b.char_root_rot; A.dof_pos = b.char_dof_pos; A.contact_forces = b.contact_forces;
    A.ref_root_pos = b.ref_root_pos; A.ref_root_rot = b.ref_root_rot; A.ref_joint_rot = b.ref_joint_rot; A.ref_contacts = b.ref_contacts;
    A.env_off = e->d_env_off;
    A.hf = e->sp.hf; A.X = e->sp.X; A.Y = e->sp.Y; A.min_x = e->sp.min_x; A.min_y = e->sp.min_y; A.dx = e->sp.dx; A.dy = e->sp.dy; A.hmax = e->hf_max;
    A.tables = e->d_tab; A.geoms = e->d_rgeom;
    A.rgba = rgba_dev; A.depth = depth_dev; A.id = id_dev;
    return PARC_OK;
}

// Headless renderer (parc_render.hpp).  Every argument is checked before the device is touched; the launch is one kernel on the caller's
// stream, outside the captured step graph, and reads the state buffers without writing any of them.
extern "C" int parc_env_render(ParcEnv *e, const ParcRenderParams *p, const int64_t *env_ids_dev, int32_t k, uint8_t *rgba_dev, float *depth_dev,
                               uint8_t *id_dev, void *stream) {
    RenderArgs A;
    PARC_TRY(render_args(e, p, "render", "the reference character needs", [&]() -> int {
        if (k < 1 || k > e->N) return fail(PARC_ERR_INVALID, "render: k must be in [1, num_envs]");
        if (k > 65535) return fail(PARC_ERR_INVALID, "render: at most 65535 envs per call");
        return PARC_OK;
    }, env_ids_dev, rgba_dev, depth_dev, id_dev, A));
    if (!rgba_dev && !depth_dev && !id_dev) return PARC_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    const dim3 grid((unsigned)((p->width + RENDER_TILE - 1) / RENDER_TILE), (unsigned)((p->height + RENDER_TILE - 1) / RENDER_TILE), (unsigned)k);
    hipLaunchKernelGGL(k_render, grid, dim3(RENDER_TILE * RENDER_TILE), 0, (hipStream_t)stream, A);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

// Scene render (parc_render_scene.hpp): one image of the characters of n envs in the one world, camera of camera_env.  Checks like
// parc_env_render before the device is touched; seven launches on the caller's stream, outside the captured step graph, reading the state
// buffers without writing any of them.  The workspace is allocated on the first call (and again when a call asks for more envs).
static int scene_stride(int B) { return (7 * B + 3) & ~3; }   // floats per character record: B rotations, B positions, 16-B aligned
static size_t scene_ws_bytes(int B, int n) {                  // per env: 2 characters x (record + sphere + key + 4 bin items)
    const size_t slots = 2 * (size_t)n;
    return sizeof(SceneHdr) + sizeof(int) * (3 * SCENE_MAX_BINS + 1) + slots * (sizeof(float) * scene_stride(B) + sizeof(float4) + sizeof(int) * (1 + SCENE_BINS_PER_SLOT));
}

extern "C" int parc_env_render_scene(ParcEnv *e, const ParcRenderParams *p, int32_t camera_env, const int64_t *env_ids_dev, int32_t n,
                                     uint8_t *rgba_dev, float *depth_dev, uint8_t *id_dev, int32_t *env_map_dev, void *stream) {
    SceneArgs S;
    memset(&S, 0, sizeof(S));
    RenderArgs &A = S.R;
    PARC_TRY(render_args(e, p, "render_scene", "the reference characters need", [&]() -> int {
        if (camera_env < 0 || camera_env >= e->N) return fail(PARC_ERR_INVALID, "render_scene: camera_env must be in [0, num_envs)");
        if (n < 1 || n > e->N) return fail(PARC_ERR_INVALID, "render_scene: n must be in [1, num_envs]");
        if (e->N > (1 << 28)) return fail(PARC_ERR_INVALID, "render_scene: at most 2^28 envs");
        return PARC_OK;
    }, env_ids_dev, rgba_dev, depth_dev, id_dev, A));
    if (!rgba_dev && !depth_dev && !id_dev && !env_map_dev) return PARC_OK;
    HIPCHK(hipSetDevice(e->cfg.device));
    if (e->scene_cap < n) {
        e->scene.release();
        e->d_scene = nullptr; e->scene_cap = 0; // a failed allocation leaves no workspace, not a stale one
        PARC_TRY(e->scene.alloc(e->d_scene, (long long)scene_ws_bytes(e->B, n)));
        e->scene_cap = n;
    }
    S.n = n; S.nk = A.draw_ref ? 2 : 1; S.cam_env = camera_env; S.stride = scene_stride(e->B); S.hmin = e->hf_min;
    S.env_map = env_map_dev;
    { // workspace carve-up (every piece 16-B aligned: the header, the bin arrays rounded up, float4 and float records first)
        const size_t slots = 2 * (size_t)e->scene_cap;
        char *w = e->d_scene;
        S.hdr = (SceneHdr *)w; w += sizeof(SceneHdr);
        S.sph = (float4 *)w; w += sizeof(float4) * slots;
        S.rec = (float *)w; w += sizeof(float) * S.stride * slots;
        S.skey = (int *)w; w += sizeof(int) * slots;
        S.items = (int *)w; w += sizeof(int) * SCENE_BINS_PER_SLOT * slots;
        S.bin_count = (int *)w; w += sizeof(int) * SCENE_MAX_BINS;
        S.bin_cursor = (int *)w; w += sizeof(int) * SCENE_MAX_BINS;
        S.bin_start = (int *)w;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned slots = (unsigned)(n * S.nk);
    hipLaunchKernelGGL(k_scene_init, dim3(1), dim3(256), 0, st, S);
    hipLaunchKernelGGL(k_scene_roots, dim3((slots + 255) / 256), dim3(256), 0, st, S);
    hipLaunchKernelGGL(k_scene_prep, dim3((slots + 63) / 64), dim3(64), 0, st, S);
    hipLaunchKernelGGL(k_scene_count, dim3((slots + 255) / 256), dim3(256), 0, st, S);
    hipLaunchKernelGGL(k_scene_scan, dim3(1), dim3(1024), 0, st, S);
    hipLaunchKernelGGL(k_scene_scatter, dim3((slots + 255) / 256), dim3(256), 0, st, S);
    const dim3 grid((unsigned)((p->width + RENDER_TILE - 1) / RENDER_TILE), (unsigned)((p->height + RENDER_TILE - 1) / RENDER_TILE));
    hipLaunchKernelGGL(k_render_scene, grid, dim3(RENDER_TILE * RENDER_TILE), 0, st, S);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

#ifdef PARC_STAMPS
// Diagnostic (-DPARC_STAMPS builds only; the shipped library does not export it): mean cycles per phase of k_env_post
// over all envs of the last step.
extern "C" int parc_env_debug_stamps(ParcEnv *e, double *mean8) {
    if (!e || !e->sp.stamp_out) return fail(PARC_ERR_STATE, "no stamp buffer");
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned> h((size_t)e->N * 8);
    HIPCHK(hipMemcpy(h.data(), e->sp.stamp_out, h.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) { double a = 0; for (int i = 0; i < e->N; ++i) a += h[(size_t)i * 8 + k]; mean8[k] = a / e->N; }
    return PARC_OK;
}
#endif

extern "C" int parc_env_profile_step(ParcEnv *e, const float *action_dev, void *stream, int32_t iters, float *avg_ms, float *avg_post_ms) {
    int rc = check_ready(e);
    if (rc) return rc;
    if (iters < 1) return fail(PARC_ERR_INVALID, "iters must be >= 1");
    double tot = 0.0, post = 0.0, dyn = 0.0;
    for (int i = 0; i < iters; ++i) {
        PARC_TRY(step_sequence(e, action_dev, (hipStream_t)stream, e->ev.ev));
        HIPCHK(hipEventSynchronize(e->ev[3]));
        float a = 0.f, b = 0.f, c = 0.f;
        PARC_TRY(e->ev.elapsed(a, 0, 3));
        PARC_TRY(e->ev.elapsed(b, 1, 2));
        PARC_TRY(e->ev.elapsed(c, 0, 1));
        tot += a; post += b; dyn += c;
    }
    if (avg_ms) *avg_ms = (float)(tot / iters);
    if (avg_post_ms) *avg_post_ms = (float)(post / iters);
    e->last_dyn_ms = (float)(dyn / iters);
    return PARC_OK;
}
