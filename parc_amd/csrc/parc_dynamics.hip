// parc_dynamics.hip — the rigid-body dynamics as a translation unit of its own: the three kernels (k_dynamics_wave and its _ff instantiation,
// k_dynamics_coop, k_dynamics) and every piece of host code that knows their tables.  The env unit (parc_env.hip) sees
// parc_dynamics_host.hpp only.  parc_build_flags() lives here: this is the unit whose flags lib.load() guards (-fno-slp-vectorize,
// -pragma-unroll-threshold: parc_dynamics_wave.hpp) and the one the test-only break-flag library rebuilds.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "parc_common.hpp"    // g_err / fail / HIPCHK / PARC_TRY, DeviceArena, dev_opt
#include "parc_dynamics.hpp"
#include "parc_dynamics_coop.hpp"
#include "parc_dynamics_host.hpp"
#include "parc_dynamics_wave.hpp"

// ------------------------------------------------------------------------------------------------
// k_dynamics: one THREAD per env advances the articulated character by one control step (nsub solver
// substeps) — clip action -> PD targets -> ABA with implicit drives and implicit cell-column contact
// (parc_dynamics.hpp).  Replaces gym.set_dof_position_target_tensor + gym.simulate x sim_steps + refresh_*
// (ig_char_env.py:488-497, ig_env.py:359-389).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_dynamics(const parcdyn::DynModel *__restrict__ M, parcdyn::DynTerrain T, ParcEnvBuffers buf,
                                                 const float *__restrict__ action, const float *__restrict__ env_off, int N) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    parcdyn::DynState S;
    S.root_pos = buf.char_root_pos + 3 * (size_t)e; S.root_rot = buf.char_root_rot + 4 * (size_t)e;
    S.root_vel = buf.char_root_vel + 3 * (size_t)e; S.root_ang_vel = buf.char_root_ang_vel + 3 * (size_t)e;
    S.dof_pos = buf.char_dof_pos + (size_t)M->D * e; S.dof_vel = buf.char_dof_vel + (size_t)M->D * e;
    S.contact_force = buf.contact_forces + (size_t)3 * M->B * e; S.body_pos = nullptr;
    parcdyn::dyn_control_step(*M, T, S, action + (size_t)M->D * e, env_off + 3 * (size_t)e);
}

// k_dynamics_wave, envs per block.  A block's latency does not depend on how many of its 64 lanes carry an env, so when 64-env blocks
// would leave half the CUs without one (a multi-GPU shard), 32-env blocks put the same work on twice the CUs: -5 % at 8 192 envs (less LDS
// and memory traffic per block; the vector instructions themselves take as long with 32 lanes as with 64)
static int wave_envs_per_block(int N, int num_cus) { return (N + 63) / 64 <= num_cus / 2 ? 32 : 64; }
// control modes vel / torque / pd_exp / pd_1d: the instantiation with the feed-forward joint torques
static auto wave_kernel(int ctrl) { return ctrl == PARC_CTRL_PD ? parcdyn::k_dynamics_wave : parcdyn::k_dynamics_wave_ff; }

struct ParcDyn {
    int N = 0, num_cus = 0;
    DeviceArena mem;                  // create .. destroy: the d_* members below are views into it
    float *d_man_ovf = nullptr;       // k_dynamics_wave: overflow area of the per-lane contact-plane lists, [blocks][4 waves][WV_MAN_OVF][8][64]
    float *d_root_shadow = nullptr;   // [N][6]: root position the dynamics last wrote + what that write rounded away (k_dynamics_wave)
    parcdyn::DynModel h_dyn;
    parcdyn::DynModel *d_dyn = nullptr;
    parcdyn::CoopTables *d_coop = nullptr;
    bool use_coop = false;
    parcdyn::WaveTables h_wave;
    parcdyn::WaveTables *d_wave = nullptr;
    bool use_wave = false, wave_rejected = false;
};

int parc_dyn_create(const ParcEnvConfig *cfg, int N, int num_cus, ParcDyn **out) {
    std::unique_ptr<ParcDyn> e(new (std::nothrow) ParcDyn()); // every failure below is a plain return: the arena releases what exists
    if (!e) return fail(PARC_ERR_INVALID, "out of host memory");
    e->N = N; e->num_cus = num_cus;
    DeviceArena &mem = e->mem;
    memset(&e->h_dyn, 0, sizeof(e->h_dyn));
    parcdyn::fill_dyn_model(e->h_dyn, cfg->model, cfg->dynamics, cfg->action_low, cfg->action_high);
    if (e->h_dyn.truncated > 0 || cfg->dynamics.num_geoms > PARC_MAX_GEOMS) // a silently shortened collision set would depend on the geom order
        return fail(PARC_ERR_INVALID, "dynamics: " + std::to_string(e->h_dyn.truncated) + " collision point(s) / segment(s) / geom(s) do not fit the model tables (DYN_MAXC " +
                    std::to_string(DYN_MAXC) + ", DYN_MAXS " + std::to_string(DYN_MAXS) + ", " + std::to_string(PARC_MAX_GEOMS) + " geoms)");
    { // control mode (ig_char_env.py:21-26, 95)
        const int cm = cfg->dynamics.control_mode;
        bool all_1d = true;
        for (int b = 1; b < cfg->model.num_bodies; ++b) all_1d = all_1d && cfg->model.joint_type[b] != parcdyn::DJ_SPHERICAL;
        if (cm < PARC_CTRL_PD || cm > PARC_CTRL_PD_1D || (cm == PARC_CTRL_PD_1D && !all_1d))
            return fail(PARC_ERR_INVALID, cm == PARC_CTRL_PD_1D ? "control_mode pd_1d only supports characters whose joints all have one dof (the reference asserts it, ig_char_env.py:246-250)"
                                                                 : "unknown control_mode " + std::to_string(cm));
    }
    // developer switches for ablation measurements (ParcEnvConfig::dev_options; the product never sets them)
    {
        const std::string mode = dev_opt(cfg, "segments"); // "none": collision points only; "capsules": drop the sole edges of boxes
        if (!mode.empty()) {
            parcdyn::DynModel &dm = e->h_dyn;
            int keep = 0;
            for (int k = 0; k < dm.nseg; ++k) {
                const bool drop = mode == "none" || (mode == "capsules" && dm.seg_r[k] <= 0.011f);
                if (drop) continue;
                dm.seg_body[keep] = dm.seg_body[k]; dm.seg_r[keep] = dm.seg_r[k];
                for (int a = 0; a < 3; ++a) { dm.seg_a[keep][a] = dm.seg_a[k][a]; dm.seg_b[keep][a] = dm.seg_b[k][a]; }
                ++keep;
            }
            dm.nseg = keep;
        }
        const std::string dt_ = dev_opt(cfg, "dtang");
        if (!dt_.empty()) e->h_dyn.dtang = (float)atof(dt_.c_str());
        const std::string mp_ = dev_opt(cfg, "man_period"); // contact discovery every n substeps (1 = every substep, the round-3 behaviour)
        if (!mp_.empty() && atoi(mp_.c_str()) >= 1) {
            e->h_dyn.man_period = atoi(mp_.c_str());
            e->h_dyn.spec_tv = 1.5f * (float)(e->h_dyn.man_period - 1) * e->h_dyn.dt;
        }
    }
    PARC_TRY(mem.alloc(e->d_dyn, 1, &e->h_dyn));
    // Kernel choice by tree shape: wave-per-limb (a trunk chain + <= 4 limb chains of <= 3 bodies, the humanoid),
    // else chain-parallel (<= 8 chains of <= 4 bodies), else thread-per-env.  PARC_DYN_KERNEL=coop|thread forces
    // one of the more general kernels (they are kept as fallbacks for other trees and as cross-checks).
    const std::string want = dev_opt(cfg, "kernel");
    parcdyn::CoopTables h_coop;
    const bool coop_ok = parcdyn::build_coop_tables(e->h_dyn, h_coop);
    const bool wave_ok = coop_ok && parcdyn::build_wave_tables(e->h_dyn, h_coop, e->h_wave);
    e->wave_rejected = !wave_ok; // the tree / the collision tables do not fit k_dynamics_wave (parc_env_describe says so: the fallbacks are several times slower)
    e->use_wave = wave_ok && want != "coop" && want != "thread";
    e->use_coop = coop_ok && !e->use_wave && want != "thread";
    if (e->use_wave) {
        PARC_TRY(mem.alloc(e->d_wave, 1, &e->h_wave));
        if (dev_opt(cfg, "no_residual").empty()) // (developer switch: the precision test measures the drift without it)
            PARC_TRY(mem.alloc_fill(e->d_root_shadow, 6LL * N, 0xff)); // NaN: matches no buffer value
        const int epb = wave_envs_per_block(N, num_cus);
        // overflow area of the contact-plane lists (never read before it is written)
        PARC_TRY(mem.alloc(e->d_man_ovf, ((long long)N + epb - 1) / epb * WV_MAXLIMB * WV_MAN_OVF * 8 * 64));
        HIPCHK(hipFuncSetAttribute((const void *)wave_kernel(e->h_dyn.ctrl), hipFuncAttributeMaxDynamicSharedMemorySize, parcdyn::wv_lds_floats() * (int)sizeof(float)));
    } else if (e->use_coop) {
        PARC_TRY(mem.alloc(e->d_coop, 1, &h_coop));
    }
    *out = e.release();
    return PARC_OK;
}

void parc_dyn_destroy(ParcDyn *d) { delete d; }

int parc_dyn_launch(const ParcDyn *e, const ParcDynTerrain &t, const ParcEnvBuffers &buf, const float *action_dev, const float *env_off, float4 *prep, hipStream_t st) {
    if (!action_dev) return fail(PARC_ERR_INVALID, "action is required when enable_dynamics is set");
    parcdyn::DynTerrain T;
    T.hf = t.hf; T.X = t.X; T.Y = t.Y; T.min_x = t.min_x; T.min_y = t.min_y; T.dx = t.dx; T.dy = t.dy;
    if (e->use_wave) {
        const int epb = wave_envs_per_block(e->N, e->num_cus);
        hipLaunchKernelGGL(wave_kernel(e->h_dyn.ctrl), dim3((e->N + epb - 1) / epb), dim3(256), parcdyn::wv_lds_floats() * sizeof(float), st,
                           (const parcdyn::DynModel *)e->d_dyn, (const parcdyn::WaveTables *)e->d_wave, T, buf, action_dev,
                           env_off, e->d_root_shadow, prep, e->d_man_ovf, e->N, epb);
    } else if (e->use_coop)
        hipLaunchKernelGGL(parcdyn::k_dynamics_coop, dim3((e->N + CO_ENVS - 1) / CO_ENVS), dim3(64), 0, st, (const parcdyn::DynModel *)e->d_dyn,
                           (const parcdyn::CoopTables *)e->d_coop, T, buf, action_dev, env_off, e->N);
    else
        hipLaunchKernelGGL(k_dynamics, dim3((e->N + 63) / 64), dim3(64), 0, st, (const parcdyn::DynModel *)e->d_dyn, T, buf, action_dev, env_off, e->N);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

bool parc_dyn_writes_prep(const ParcDyn *e) { return e->use_wave; } // k_dynamics_wave writes the prep records with the state

std::string parc_dyn_describe(const ParcDyn *e) {
    char b[1024];
    std::string d;
    const parcdyn::DynModel &m = e->h_dyn;
    snprintf(b, sizeof(b), "dynamics_kernel=%s;", e->use_wave && m.ctrl != PARC_CTRL_PD ? "k_dynamics_wave_ff" : parc_dyn_kernel_name(e)); d += b;
    static const char *const ctrl_names[] = {"pd", "vel", "torque", "pd_exp", "pd_1d"};
    snprintf(b, sizeof(b), "control_mode=%s;", ctrl_names[m.ctrl]); d += b;
    snprintf(b, sizeof(b), "envs_per_block=%d;substeps=%d;substep_dt=%.9g;collision_points=%d;collision_segments=%d;kn=%g;dn=%g;dtang=%g;mu=%g;pen_cap=%g;"
             "manifold_period=%d;spec_m0=%g;spec_tv=%g;spec_max=%g;root_residual=%d;", e->use_wave ? wave_envs_per_block(e->N, e->num_cus) : (e->use_coop ? CO_ENVS : 64),
             m.nsub, (double)m.dt, m.ncol, m.nseg, (double)m.kn, (double)m.dn, (double)m.dtang, (double)m.mu, (double)m.pen_cap, m.man_period, (double)m.spec_m0,
             (double)m.spec_tv, (double)m.spec_max, e->d_root_shadow ? 1 : 0);
    d += b;
    if (e->wave_rejected) d += "note=the model does not fit k_dynamics_wave (tree shape or > 32 candidates on a body): general fallback kernel;";
    if (e->use_wave) { snprintf(b, sizeof(b), "manifold_lds_slots=%d+%d+%d+%d;manifold_overflow_slots=%d;", e->h_wave.man_cap[0], e->h_wave.man_cap[1], e->h_wave.man_cap[2], e->h_wave.man_cap[3], WV_MAN_OVF); d += b; }
    return d;
}

const char *parc_dyn_kernel_name(const ParcDyn *e) { return e->use_wave ? "k_dynamics_wave" : (e->use_coop ? "k_dynamics_coop" : "k_dynamics"); }

int parc_dyn_counters(ParcDynCounters *c) {
    HIPCHK(hipGetSymbolAddress((void **)&c->timeouts, HIP_SYMBOL(parcdyn::g_wave_timeouts)));
    HIPCHK(hipGetSymbolAddress((void **)&c->man_drops, HIP_SYMBOL(parcdyn::g_wave_man_drops)));
    return PARC_OK;
}

// Both must stay 0: a timed-out wait poisons its block's envs (parc_dynamics_wave.hpp), a dropped plane (the per-lane list's LDS share +
// overflow area were full; WvMan) is a contact the substeps after a discovery do not see.
int parc_dyn_read_counter(bool man_drops) {
    ParcDynCounters c;
    unsigned int v = 0;
    PARC_TRY(parc_dyn_counters(&c));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(&v, man_drops ? c.man_drops : c.timeouts, sizeof(v), hipMemcpyDeviceToHost));
    return (int)(v > 0x7fffffffu ? 0x7fffffffu : v);
}

#ifndef PARC_BUILD_FLAGS
#define PARC_BUILD_FLAGS "unknown"
#endif
extern "C" const char *parc_build_flags(void) { return PARC_BUILD_FLAGS; }

#if defined(PARC_STAMPS) || defined(PARC_TIMELINE)
// Diagnostic builds only (the shipped library exports none of these): the n 64-bit counters of a device symbol since the last call,
// cleared by the call unless `keep`.
static int read_counters(const void *symbol, int n, double *out, bool keep = false) {
    const std::vector<unsigned long long> z((size_t)n, 0ull);
    std::vector<unsigned long long> h((size_t)n);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(h.data(), symbol, sizeof(unsigned long long) * n));
    if (!keep) HIPCHK(hipMemcpyToSymbol(symbol, z.data(), sizeof(unsigned long long) * n));
    for (int i = 0; i < n; ++i) out[i] = (double)h[i];
    return PARC_OK;
}
#endif
#ifdef PARC_STAMPS
// cycles per phase of k_dynamics_coop, summed over all waves
extern "C" int parc_env_debug_dyn_stamps(double *out16) { return read_counters(&parcdyn::g_dyn_stamps, 16, out16); }
// cycles per segment of k_dynamics_wave, per wave role [4][16], summed over all blocks
extern "C" int parc_env_debug_wave_stamps(double *out64) { return read_counters(&parcdyn::g_wave_stamps, 64, out64); }
// contact-cull statistics of k_dynamics_wave per body [16][8] (see g_wave_cnt)
extern "C" int parc_env_debug_wave_counts(double *out128) { return read_counters(&parcdyn::g_wave_cnt, 128, out128); }
// manifold-size histograms of k_dynamics_wave [16][4][16] (see g_wave_hist; -DPARC_COUNTS builds fill them)
extern "C" int parc_env_debug_wave_hist(double *out1024) { return read_counters(&parcdyn::g_wave_hist, 1024, out1024); }
#endif
#ifdef PARC_TIMELINE
// absolute cycle counter at the hand-off points of one substep of block 0, [wave][event]: not cleared
extern "C" int parc_env_debug_wave_timeline(double *out64) { return read_counters(&parcdyn::g_wave_tl, 64, out64, true); }
#endif
