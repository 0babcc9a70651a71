// parc_dynamics_host.hpp — all the env unit (parc_env.hip) knows of the rigid-body dynamics: declarations only, defined in
// parc_dynamics.hip.  No kernel header is included here, so an edit of a dynamics kernel does not recompile the env unit and an edit of
// the env unit does not recompile k_dynamics_wave.  Every function runs on the current device and reports through fail() / parc_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/parc_env.h"

struct ParcDyn;   // the model tables, the kernel choice, the root shadow and the manifold overflow area; its device memory is an arena of its own

struct ParcDynTerrain {   // the heightfield the characters collide with (parc_env_load_terrain)
    const float *hf;
    int X, Y;
    float min_x, min_y, dx, dy;
};

// cfg->enable_dynamics is set.  Validates the model (collision tables, control mode), applies the developer switches of cfg->dev_options
// (segments, dtang, man_period, kernel, no_residual) and picks the kernel for N envs on a device of num_cus compute units.
int parc_dyn_create(const ParcEnvConfig *cfg, int N, int num_cus, ParcDyn **out);
void parc_dyn_destroy(ParcDyn *d);   // null is fine
// one control step of all N envs; `prep` = the [N][16] prep records of k_env_post, written when parc_dyn_writes_prep()
int parc_dyn_launch(const ParcDyn *d, const ParcDynTerrain &T, const ParcEnvBuffers &buf, const float *action, const float *env_off, float4 *prep, hipStream_t st);
bool parc_dyn_writes_prep(const ParcDyn *d);
std::string parc_dyn_describe(const ParcDyn *d);   // the "dynamics_kernel=...;...;" part of parc_env_describe
const char *parc_dyn_kernel_name(const ParcDyn *d);

// The two health counters of k_dynamics_wave, one pair per process and device: flag waits that timed out, contact planes that found no slot.
struct ParcDynCounters { const unsigned int *timeouts, *man_drops; };   // device addresses
int parc_dyn_counters(ParcDynCounters *c);      // the curriculum kernels publish the pair through them
int parc_dyn_read_counter(bool man_drops);      // one counter's value once the device is idle, at most INT_MAX (< 0: error code)
