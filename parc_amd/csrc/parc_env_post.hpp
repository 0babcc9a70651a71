// parc_env_post.hpp — the step path of the env: k_env_prep and k_env_post (observation, reward, done), with their macros and wave helpers.
//
// One wavefront (64 lanes) owns one environment:
//   * the joint hierarchy / per-body tables are staged once per wave into LDS;
//   * the 8 skeletons of a step (character, reference, 6 look-ahead targets) are 8 rows of 16 lanes:
//     lane (row, i) produces quaternion i of that row (slerp of two 512-byte frame records, or
//     dof->quat for the character) and its tan-norm observation in the same instruction stream;
//   * FK runs one root-to-leaf chain per lane (8 rows x 8 chains), no cross-lane traffic;
//   * the 441 height rays read a (2r+1)^2 terrain tile staged in LDS;
//   * the 1312-float observation row is assembled in LDS and streamed out as 16-byte stores.
// No MFMA: the work is quaternion algebra and gathers.  HBM traffic per env-step is the state read
// (456 B + 24 B bookkeeping) and the observation/reward write (5.3 KB); motion records and the terrain
// grid stay cache resident.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/parc_env.h"
#include "parc_common.hpp"       // MotionMeta, Blend, frame_blend
#include "parc_env_tables.hpp"   // StepParams, DevTables, REC_*, cell_index*, list_env, prep_record_slot
#include "parc_lanetab.hpp"      // prefetch phase, heading pass and contact block of k_env_post: what depends on the lane and on the handle's constants only
#include "parc_math.hpp"
#include "parc_rowmap.hpp"       // row phase of k_env_post: (pass, lane) -> (row, slot)

// ------------------------------------------------------------------------------------------------
// k_env_prep: the work that is scalar per env and transcendental-heavy — heading, inverse heading quaternion,
// cos/sin of the heading for the ray fan, and dof -> joint quaternion of the character (kin_char_model.py:586;
// torch_util.py:502-530).  In the wave-per-env kernel these would run with 15 of 64 lanes (measured: +35 us at 65 536
// envs when folded in, against the 22 us of this kernel); here all lanes are busy.  Output: a 256-byte record per env
// (L2 / Infinity-Cache resident between the two launches).  The kernels that WRITE the state form the same record with the
// same device functions (k_dynamics_wave after a step, k_reset_with after a reset); this kernel runs when the caller owns
// the state (parc_env_compute_obs, physics off) or one of the fallback dynamics kernels stepped it.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_env_prep(const StepParams P, const int64_t *__restrict__ env_ids,
                                                 const int *__restrict__ env_ids32, const int *__restrict__ count_dev, int count) {
    // 16 lanes per env (4 envs per wave): lane 0 forms the heading terms, lane j the quaternion of joint j.  One
    // transcendental chain per lane instead of fifteen per thread: the same instruction count at 65 536 envs, a 10x shorter
    // critical path at the few thousand envs of a multi-GPU shard.
    if (count_dev) count = *count_dev;
    const int it = blockIdx.x * 4 + (threadIdx.x >> 4), j = threadIdx.x & 15;
    if (it >= count || j >= P.B) return;
    const int e = list_env(env_ids, env_ids32, it);
    const float4 *root_rot = (const float4 *)(P.buf.char_root_rot + 4 * (size_t)e); // read by slot 0 alone
    P.prep[(size_t)e * 16 + j] = prep_record_slot(P.tables, j, *root_rot, P.buf.char_dof_pos + (size_t)e * P.D);
}

// ------------------------------------------------------------------------------------------------
// the step kernel: IGEnv._post_physics_step (ig_env.py:368-377), one env per wave, four envs per 256-thread workgroup
// ------------------------------------------------------------------------------------------------
// Diagnostic build only (-DPARC_STAMPS): per-phase s_memtime stamps of lane 0 go to a debug buffer that no
// other code reads; the shipped library is built without it.
#ifdef PARC_STAMPS
#define STAMP(i) do { if (lane == 0) s_stamp[i] = __builtin_readcyclecounter(); } while (0)
#else
#define STAMP(i) do { } while (0)
#endif
#define MODE_STEP 0
#define MODE_OBS 1
#define ENVS_PER_BLOCK 4
// orders the LDS traffic of ONE wave (see k_env_post): a compiler-level fence, no instruction
#define WAVE_SYNC() asm volatile("" ::: "memory")
#define RAY_UNROLL 8

__device__ __forceinline__ float wave_sum(float v) { // butterfly over the 64 lanes; every lane gets the total
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// Sum within each 16-lane row with four DPP row rotations (no LDS crossbar traffic): every lane of a row ends up with its row's total.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float v) {
    v = v + dpp_f32<0x128>(v); // row_ror:8
    v = v + dpp_f32<0x124>(v); // row_ror:4
    v = v + dpp_f32<0x122>(v); // row_ror:2
    v = v + dpp_f32<0x121>(v); // row_ror:1
    return v;
}
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// MIRROR = false: none of the optional outputs (the ref_* mirrors of the reference's tensors, ray_hfs, tracking_error) is bound --
// the training configuration.  Their pointers and null checks then leave the kernel (20+ SGPRs: the kernel is at the SGPR limit and every
// scalar spilled to a VGPR lane comes back as a VALU instruction).
// LOCALROOT = the config's `track_root: false`: the reward compares root rotation, root velocities and key positions in each character's
// own heading frame (convert_to_local, mgdm_dm_util.py:247-267).  An instantiation of its own so that the default one carries none of it.
// OBSVAR = a non-default observation layout, decided at run time inside these instantiations only: `global_obs: true` (P.global_obs: the
// character and target observations stay in the global frame -- no heading rotation, the targets' key offsets are not shifted by the root
// offset) and / or `global_root_height_obs: true` (P.off_char = 1: the root height in front of the character block).  Instantiated with
// MIRROR = true only (off the default path).
template <int MODE, bool MIRROR, bool LOCALROOT = false, bool OBSVAR = false>
__global__ __launch_bounds__(256, 5) void k_env_post(const StepParams P, const int64_t *__restrict__ env_ids,
                                                 const int *__restrict__ env_ids32, const int *__restrict__ count_dev, int count,
                                                 unsigned long long *bump_calls) {
    // P arrives by value in the kernarg segment: its pointers are then known to be global (global_load / global_store
    // instead of flat_*, which would also tie up the LDS wait counter), its scalars are scalar loads where they are used
    // A workgroup is four waves = four envs (ENVS_PER_BLOCK).  Everything up to the reward is wave-private: each wave owns slice `wv` of
    // the LDS arrays and orders its own LDS traffic with WAVE_SYNC (LDS executes a wave's instructions in order; only the compiler has
    // to be kept from moving a read above the write of another lane).  The joint hierarchy is staged by every wave with the same values.
    extern __shared__ __align__(16) float s_obs_all[]; // per wave: staged observation prefix [0, off_tarc) (+ the body rotations of the tracking error)
    __shared__ int s_tab_raw[HIER_STAGED_WORDS];
    const HierTables &s_tab = *reinterpret_cast<const HierTables *>(s_tab_raw); // only the staged members are touched through it
    // One block per wave, so that the heading pass addresses any of its float4 with one offset of its table (parc_lanetab.hpp, PARC_HROT_*_F4):
    //   s_q  [8][16]  row r: quats 0..14 (0 = root), slot 15 = root position.  Target rows (r >= 2) hold lr (x) q for the joints
    //   s_fk [80]     FK positions: rows 0,1 all bodies [r*16+b]; target rows key slots [32+(r-2)*8+k]
    //   s_rv [4]      root velocity and root angular velocity of the character as loaded, a zero vector, one spare
    __shared__ float4 s_blk_all[ENVS_PER_BLOCK][PARC_HROT_BLOCK_F4];
    __shared__ float4 s_lq_all[ENVS_PER_BLOCK][2][16];  // rows 0, 1: lr (x) q of the joints (s_q keeps their raw quaternions for the reward)
    // (LDS budget: 864 B of tables + 4 x (4 432 B static + 3 072 B staged row) = 30.2 KB per workgroup: 5 workgroups = 5 waves per SIMD
    // on a CU's 160 KB)
    __shared__ float s_cdofv_all[ENVS_PER_BLOCK][PARC_MAX_DOFS];
    __shared__ float4 s_refvel_all[ENVS_PER_BLOCK][12]; // record float4 #20..: root_vel, root_ang_vel, dof_vel
    __shared__ __align__(16) float s_refct_all[ENVS_PER_BLOCK][16];
    __shared__ float s_cfn_all[ENVS_PER_BLOCK][16];
    __shared__ float s_sc_all[ENVS_PER_BLOCK][16];      // per-env scalars handed to the wave that forms the rewards (MODE_STEP)
#ifdef PARC_STAMPS
    __shared__ unsigned long long s_stamp_all[ENVS_PER_BLOCK][16];
#endif
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const bool GLOBALOBS = OBSVAR && P.global_obs != 0; // a compile-time false in the default instantiations
    const int oc = OBSVAR ? P.off_char : 0;              // offset of the character block (1 when the root height leads the row)
    const bool TAROBS = !OBSVAR || P.obs_tar != 0;       // enable_tar_obs (ig_parkour_env.py:83): the look-ahead target block exists
    const bool CONTACTOBS = !OBSVAR || P.obs_contact != 0; // use_contact_info (:72): contact blocks of the observation, contact term of the reward
    float *s_obs = s_obs_all + (size_t)wv * P.lds_wave_floats;
    float4 (*s_q)[16] = reinterpret_cast<float4 (*)[16]>(s_blk_all[wv] + PARC_HROT_Q_F4);
    float4 (*s_lq)[16] = s_lq_all[wv];
    float4 *s_fk = s_blk_all[wv] + PARC_HROT_FK_F4;
    float4 *s_rv = s_blk_all[wv] + PARC_HROT_RV_F4;
    float4 *s_cbp = s_lq[0];        // simulator rigid-body positions of the character: written once the FK chains are through with s_lq
    float *s_cdofv = s_cdofv_all[wv];
    float4 *s_refvel = s_refvel_all[wv];
    float *s_refct = s_refct_all[wv], *s_cfn = s_cfn_all[wv];
#ifdef PARC_STAMPS
    unsigned long long *s_stamp = s_stamp_all[wv];
#endif
    float *s_tile = (float *)s_fk;  // the terrain tile is dead before FK writes s_fk
    float4 (*s_br)[16] = reinterpret_cast<float4 (*)[16]>(s_obs + ((P.off_tarc + 3) & ~3)); // body rotations of char/ref: only allocated
                                                                                            // (behind the staged prefix) when the tracking error is reported

    // the observation pass of a sampling reset closes the call: every block of the reset kernel has read the Philox call index by now
    if (MODE == MODE_OBS && bump_calls && blockIdx.x == 0 && threadIdx.x == 0) *bump_calls += 1ull;
    if (count_dev) count = *count_dev; // device-side list (reset_done): no host round trip
    const int it = blockIdx.x * ENVS_PER_BLOCK + wv;
    if (it >= count) return;
    int e = list_env(env_ids, env_ids32, it);
    e = __builtin_amdgcn_readfirstlane(e);
    STAMP(0);

    const int B = P.B, D = P.D, S = P.S, K = P.K, J = P.J;
    const DevTables *__restrict__ T = P.tables;

    float *orow = P.buf.obs + (size_t)e * P.obs_dim;

    // ================= prefetch: every global load of this env is issued before any is consumed =================
    // (a) loads that only need the env id go first, so they overlap the scalar bookkeeping chain below
    constexpr int HW = HIER_STAGED_WORDS;
    constexpr int HN = (HW + 63) / 64;
    int tabreg[HN];
#pragma unroll
    for (int i = 0; i < HN; ++i) { const int w = lane + 64 * i; tabreg[i] = w < HW ? ((const int *)&T->h)[w] : 0; }
    // the lane's table entry (parc_lanetab.hpp): the address needs the lane only.  Every index it yields is in bounds on every lane, so
    // the loads below carry no branch and no default; a lane without an item loads a neighbour's value that nothing consumes
    unsigned lt[PARC_LANETAB_WORDS];
    {
        static_assert(sizeof(ParcLaneEntry) == sizeof(uint4), "one 16-byte load per lane");
        const uint4 l0 = *reinterpret_cast<const uint4 *>(T->lane + lane);
        lt[0] = l0.x; lt[1] = l0.y; lt[2] = l0.z; lt[3] = l0.w;
    }
    const float dofv = P.buf.char_dof_vel[(size_t)e * D + parc_lt_dof(lt)];
    const unsigned role = parc_lt_role(lt); // lanes 32..32+B: contact force; 30/31: root (ang) vel
    float aux0, aux1, aux2;
    {
        const float *src = P.buf.contact_forces + 3 * (size_t)e * B + parc_lt_force_off(lt);
        src = role == PARC_LT_ROLE_ROOT_VEL ? P.buf.char_root_vel + 3 * (size_t)e : src;
        src = role == PARC_LT_ROLE_ROOT_ANG_VEL ? P.buf.char_root_ang_vel + 3 * (size_t)e : src;
        aux0 = src[0]; aux1 = src[1]; aux2 = src[2];
    }
    // the lane's (row, slot) item of the two row passes (parc_rowmap.hpp): pass A = every root item + the first 48 joint items, pass B = joints
    // as row * 16 + slot, -1 = none (one register per pass is all the row phase keeps across the ray loop)
    const int item[2] = {parc_lt_item(lt, 0), parc_lt_item(lt, 1)};
    // slot 0 heading terms (lane 0), 1..B-1 character joint quats (k_env_prep): row 0's items all sit in pass A, where the record slot
    // of a row-0 lane is its slot of this record too (lane 0: slot 0, read back by every lane below)
    const float4 prepq = P.prep[(size_t)e * 16 + parc_lt_row_slot(lt, 0)];
    float2 rayp[RAY_UNROLL];
    // ray lane + 64 i, clamped to the last ray (parc_lt_ray_off).  A slot wholly past R (top < 0, i.e. 64 i >= R) is not loaded and stays
    // unset: the ray loop reads slot i under `base + 64 * i < P.R` (tile path) or `r < P.R` (gathers) only, which imply top >= 0
#pragma unroll
    for (int i = 0; i < RAY_UNROLL; ++i) {
        const int top = parc_lt_ray_top(P.R, i); // uniform
        if (top >= 0) rayp[i] = *(const float2 *)((const char *)P.ray_points + parc_lt_ray_off(lane, i, top));
    }

    // (b) bookkeeping + time (ig_env.py:391-394, dm_env.py:547-552): uniform, scalar loads
    const int mid = P.buf.motion_ids[e];
    const int tid = P.buf.terrain_ids[e];
    const float toff = P.buf.time_offsets[e];
    int ts = P.buf.timestep[e];
    if (MODE == MODE_STEP) ts += 1;
    const float time = P.dt_f * (float)ts;
    const float mt = time + toff;
    const MotionMeta meta = P.meta[mid];
    const float eox = P.env_offsets[3 * e + 0], eoy = P.env_offsets[3 * e + 1], eoz = P.env_offsets[3 * e + 2];
    const float *mo = P.motion_offsets + 2 * ((size_t)mid * P.T + tid);
    const float offx = mo[0] - eox, offy = mo[1] - eoy; // dm_env.py:556
    const float *crp = P.buf.char_root_pos + 3 * (size_t)e;
    const float *crr = P.buf.char_root_rot + 4 * (size_t)e;
    const V3 root_pos = mk3(crp[0], crp[1], crp[2]);
    const Q4 root_rot = mk4(crr[0], crr[1], crr[2], crr[3]);
    const float gx = root_pos.x + eox, gy = root_pos.y + eoy, gz = root_pos.z + eoz; // ig_parkour_env.py:522

    // (c) reference motion: rows 1..1+S (the lane's item of each row pass), two 512-byte frame records per sample.  The frame pair and blend factor
    // of a sample (motion_lib.py:425-438) are formed once, by lane (sample & 7): sample 0 = the reference at t, sample s = look-ahead
    // target s; the row / contact / velocity lanes fetch theirs with a lane shuffle instead of evaluating the blend four times per lane.
    Blend myb;
    {
        const int sid = lane & 7;
        float t = mt;
#pragma unroll
        for (int q = 0; q < PARC_MAX_TAR_STEPS; ++q) t = (sid - 1 == q) ? mt + P.tstep[q] : t;
        myb = frame_blend(meta, t);
    }
    const int last_frame = meta.start + meta.nframes - 1;
    float4 fA[2], fB[2];
    Blend bl[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int src4 = (int)parc_lt_src4(lt, p); // 4 x the sample of the item's row (sample 0 on row 0 and on a lane without an item)
        bl[p].b = __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(myb.b)));
        bl[p].i0 = __builtin_amdgcn_ds_bpermute(src4, myb.i0);
        bl[p].i1 = min(bl[p].i0 + 1, last_frame); // = frame_blend's i1
        const unsigned slot = parc_lt_row_slot(lt, p);
        fA[p] = P.records[(size_t)bl[p].i0 * REC_F4 + slot];
        fB[p] = P.records[(size_t)bl[p].i1 * REC_F4 + slot];
    }
    // (d) contacts of the 1+S samples (lanes < 4(1+S)) / velocity block of sample 0 (lanes 32..)
    // (every other lane: contact slot 0 of sample 0)
    const int src4c = (int)parc_lt_src4(lt, 2);
    const float cblend = __int_as_float(__builtin_amdgcn_ds_bpermute(src4c, __float_as_int(myb.b)));
    const int b2i0 = __builtin_amdgcn_ds_bpermute(src4c, myb.i0), b2i1 = min(b2i0 + 1, last_frame);
    const float4 cA = P.records[(size_t)b2i0 * REC_F4 + parc_lt_cv_slot0(lt)]; // velocities come from frame idx0 un-interpolated (:103-109)
    const float4 cB = P.records[(size_t)b2i1 * REC_F4 + parc_lt_cv_slot1(lt)];
    // (e) terrain tile cells: (a, bq) of the lane's five cells from the table, (0, 0) where the tile ends (or there is none: tr < 0)
    static_assert(64 * PARC_LANETAB_TILE_CELLS == TILE_MAX_CELLS && TILE_MAX_CELLS * sizeof(float) == (PARC_HROT_RV_F4 - PARC_HROT_FK_F4) * sizeof(float4), "the five tile stores of a lane stay inside s_fk");
    const int tr = P.tile_r, TW = 2 * tr + 1;
    // (the origin is kept within +-2^22 cells so that it and the tile bounds are exact as floats: the ray loop clamps in float)
    const int ox = min(max(cell_index(gx, P.min_x, P.dx) - tr, -(1 << 22)), 1 << 22), oy = min(max(cell_index(gy, P.min_y, P.dy) - tr, -(1 << 22)), 1 << 22);
    float tilev[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int cx = min(max(ox + (int)parc_lt_cell_a(lt, i), 0), P.X - 1), cy = min(max(oy + (int)parc_lt_cell_b(lt, i), 0), P.Y - 1);
        tilev[i] = P.hf[(size_t)cx * P.Y + cy];
    }

    // ================= heading terms from k_env_prep (uniform), LDS fills =================
    const float ch = __shfl(prepq.x, 0, 64), sh = __shfl(prepq.y, 0, 64);
    const Q4 hinv = mk4(0.f, 0.f, __shfl(prepq.z, 0, 64), __shfl(prepq.w, 0, 64)); // axis_angle_to_quat(z, -heading): x = y = 0 exactly
#pragma unroll
    for (int i = 0; i < HN; ++i) { const int w = lane + 64 * i; if (w < HW) s_tab_raw[w] = tabreg[i]; }
    if (lane < D) {
        s_cdofv[lane] = dofv;
        s_obs[P.off_dofvel + lane] = dofv;
    }
    if (OBSVAR && oc && lane == 29) s_obs[0] = root_pos.z; // root_height_obs (ig_char_env.py:620-622)
    // root velocities as loaded (roles 1, 2 -> s_rv[0], s_rv[1]): the heading pass rotates them, the reward reads them; lane 29 lays down
    // the zero vector that the pass subtracts from them
    static_assert(PARC_LT_ROLE_ROOT_VEL == 1 && PARC_LT_ROLE_ROOT_ANG_VEL == 2 && PARC_HROT_RV_ZERO == 2, "s_rv slots");
    if (role == PARC_LT_ROLE_ROOT_VEL || role == PARC_LT_ROLE_ROOT_ANG_VEL) s_rv[role - 1] = make_float4(aux0, aux1, aux2, 0.f);
    if (lane == 29) s_rv[PARC_HROT_RV_ZERO] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (role == PARC_LT_ROLE_FORCE) { // contact flags + clamped force norms (ig_parkour_env.py:655-662, mgdm_dm_util.py:505-508)
        const float n = norm3(mk3(aux0, aux1, aux2));
        if (CONTACTOBS) orow[P.off_cc + (lane - 32)] = n > 1e-5f ? 1.f : 0.f;
        s_cfn[lane - 32] = fminf(n, 1.0f);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) s_tile[lane + 64 * i] = tilev[i]; // past the tile's last cell: scratch that FK overwrites
    WAVE_SYNC();
    STAMP(1);

    // ================= height rays (mgdm_dm_util.py:128-145; terrain_util.py:146-156) =================
    // Two loops, one per source of the heights, so that the common one reads the LDS tile with plain ds_read (a pointer that may
    // be LDS or global becomes a flat load, whose wait also covers the stores of the previous ray).
    {
        float *hrow = orow + P.off_hf;
        float *hmirror = MIRROR && P.buf.ray_hfs ? P.buf.ray_hfs + (size_t)e * P.R : nullptr;
        for (int base = 0; base < P.R; base += 64 * RAY_UNROLL) {
            if (base > 0) {
#pragma unroll
                for (int i = 0; i < RAY_UNROLL; ++i) { const int r = base + lane + 64 * i; rayp[i] = r < P.R ? ((const float2 *)P.ray_points)[r] : make_float2(0.f, 0.f); }
            }
            const float tlox = (float)ox, thix = (float)(ox + TW - 1), tloy = (float)oy, thiy = (float)(oy + TW - 1);
            if (tr >= 0) { // the tile radius covers the whole fan by construction (parc_env_load_terrain): clamp, no fallback
                // every tile index is formed before the first store: a later use of a loaded ray point would have to wait for
                // the stores issued in between (one counter orders loads and stores).  Lanes past the end of the fan carry the
                // point (0, 0), a valid cell; only their stores are masked.
                int tix[RAY_UNROLL];
#pragma unroll
                for (int i = 0; i < RAY_UNROLL; ++i) {
                    tix[i] = 0;
                    if (base + 64 * i < P.R) { // uniform; for base = 0 the condition under which the prefetch loaded rayp[i]
                        const float px = (rayp[i].x * ch - rayp[i].y * sh) + gx; // rotate_2d_vec torch_util.py:651
                        const float py = (rayp[i].x * sh + rayp[i].y * ch) + gy;
                        // nearest cell (cell_index_rcp), clamped to the tile while still a float: the bounds are small integers, so
                        // clamp-then-convert equals convert-then-clamp and the guard against a wild float comes for free
                        const int a = (int)fminf(fmaxf(cell_float_rcp(px, P.min_x, P.dx, P.rdx), tlox), thix) - ox;
                        const int bq = (int)fminf(fmaxf(cell_float_rcp(py, P.min_y, P.dy, P.rdy), tloy), thiy) - oy;
                        tix[i] = a * TW + bq;
                    }
                    asm volatile("" : "+v"(tix[i])); // keep the index arithmetic here (not sunk below the stores)
                }
                float hv[RAY_UNROLL];
#pragma unroll
                for (int i = 0; i < RAY_UNROLL; ++i) hv[i] = s_tile[tix[i]]; // one batch of LDS reads, one wait
#pragma unroll
                for (int i = 0; i < RAY_UNROLL; ++i) {
                    const int r = base + lane + 64 * i;
                    if (r < P.R) {
                        float h = hv[i] - gz;
                        h = fminf(fmaxf(h, P.min_obs_h), P.max_obs_h);
                        hrow[r] = h; // 256 contiguous bytes per wave store: no staging needed
                        if (hmirror) hmirror[r] = h;
                    }
                }
            } else { // fan too wide for the LDS tile: direct gathers
#pragma unroll
                for (int i = 0; i < RAY_UNROLL; ++i) {
                    const int r = base + lane + 64 * i;
                    if (r < P.R) {
                        const float px = (rayp[i].x * ch - rayp[i].y * sh) + gx;
                        const float py = (rayp[i].x * sh + rayp[i].y * ch) + gy;
                        const int ix = cell_index_rcp(px, P.min_x, P.dx, P.rdx), iy = cell_index_rcp(py, P.min_y, P.dy, P.rdy);
                        const int cx = min(max(ix, 0), P.X - 1), cy = min(max(iy, 0), P.Y - 1);
                        float h = P.hf[(size_t)cx * P.Y + cy] - gz;
                        h = fminf(fmaxf(h, P.min_obs_h), P.max_obs_h);
                        hrow[r] = h;
                        if (hmirror) hmirror[r] = h;
                    }
                }
            }
        }
    }
    STAMP(2);

    // ================= row items: quaternions of char / ref / targets + tan-norm observations =================
    // One body for both passes.  ROOT (pass A) carries the code of the root items (slot 0 = root rotation, slot 15 = root position: the
    // position lerp with its loop and terrain offsets, the heading products) and of rows 0 and 1, whose joints all sit in pass A; pass B
    // is compiled without any of it: joint items of target rows only.
    static_assert(2 * (PARC_MAX_BODIES - 2) <= PARC_ROWMAP_JOINTS_A, "the joints of rows 0 and 1 must fit into pass A");
    // the lane's item of the heading pass and its part in the contact / velocity block (parc_lanetab.hpp): loaded here, behind the ray loop;
    // word 2 is consumed after the row passes, words 0 and 1 once the FK chains are through
    unsigned hr[3];
    {
        const unsigned *h0 = T->hrot[lane].w; // one 12-byte load per lane
        hr[0] = h0[0]; hr[1] = h0[1]; hr[2] = h0[2];
    }
    auto row_pass = [&](auto root_tag, const int itm, const float4 A, const float4 Bv, const float bb) {
        constexpr bool ROOT = decltype(root_tag)::value;
        if (itm < 0) return;
        const int r = itm >> 4, i = itm & 15;
        const bool is_rot = ROOT && i == 0, is_pos = ROOT && i == 15;
        const bool row0 = ROOT && r == 0, row1 = ROOT && r == 1;
        float4 res = make_float4(0.f, 0.f, 0.f, 1.f);
        if (row0) { // character: dof -> quat (kin_char_model.py:586)
            if (is_rot) res = root_rot;
            else if (is_pos) res = make_float4(root_pos.x, root_pos.y, root_pos.z, 0.f);
            else res = prepq;
        } else { // reference motion sample (motion_lib.py:94-128)
            if (is_pos) {
                const float a = 1.0f - bb;
                res.x = a * A.x + bb * Bv.x;
                res.y = a * A.y + bb * Bv.y;
                res.z = a * A.z + bb * Bv.z;
                res.w = 0.f;
                if (meta.loop == PARC_LOOP_WRAP) { // _calc_loop_offset :440
                    float t = mt;
#pragma unroll
                    for (int q = 0; q < PARC_MAX_TAR_STEPS; ++q) t = (r - 2 == q) ? mt + P.tstep[q] : t;
                    const float ph = floorf(t / meta.length);
                    res.x = res.x + ph * meta.dx; res.y = res.y + ph * meta.dy; res.z = res.z + ph * meta.dz;
                }
                res.x = res.x + offx; // _move_to_motion_terrain dm_env.py:554
                res.y = res.y + offy;
            } else {
                res = slerp_rr(A, Bv, bb);
            }
        }
        if (!is_rot && !is_pos) { // the FK chains multiply parent (x) (lr (x) q): the inner product is formed here, once per joint,
                                  // instead of once per chain level (same operations, same order)
            const Q4 lq = P.lr_identity ? res : quat_mul(mk4(s_tab.lr[i][0], s_tab.lr[i][1], s_tab.lr[i][2], s_tab.lr[i][3]), res);
            if (row0 || row1) { s_lq[r][i] = lq; s_q[r][i] = res; } else s_q[r][i] = lq;
        } else {
            s_q[r][i] = res;
        }
        if (row1) { // optional mirrors of the reference's ref_* tensors
            if (MIRROR && is_rot && P.buf.ref_root_rot) *(float4 *)(P.buf.ref_root_rot + 4 * (size_t)e) = res;
            if (MIRROR && !is_rot && !is_pos && P.buf.ref_joint_rot) *(float4 *)(P.buf.ref_joint_rot + 4 * ((size_t)e * J + i - 1)) = res;
            if (MIRROR && is_pos && P.buf.ref_root_pos) {
                float *o = P.buf.ref_root_pos + 3 * (size_t)e;
                o[0] = res.x; o[1] = res.y; o[2] = res.z;
            }
        } else if (row0 || TAROBS) { // observation pieces (ig_char_env.py:582, mgdm_dm_util.py:405)
            const int base = row0 ? 0 : P.off_tar + (r - 2) * P.tar_w;
            if (!is_pos) {
                const Q4 qq = (is_rot && !GLOBALOBS) ? quat_mul(hinv, res) : res;
                float tn[6];
                quat_to_tan_norm(qq, tn);
                const int o = row0 ? oc + (is_rot ? 0 : 12 + 6 * (i - 1)) : base + 3 + 6 * i;
#pragma unroll
                for (int c = 0; c < 6; ++c) s_obs[o + c] = tn[c];
            } // (a target row's root offset: the heading pass, from s_q[r][15])
        }
    };
    row_pass(std::true_type(), item[0], fA[0], fB[0], bl[0].b);
    row_pass(std::false_type(), item[1], fA[1], fB[1], bl[1].b);
    // ---- contacts of the 1+S samples and the velocity block of sample 0 ---------------------------------
    // (which lane does what, how many of its four contacts are bodies and where they go: word 2 of the lane's heading-table entry)
    const unsigned cvk = parc_hr_cv_kind(hr);
    if (cvk == PARC_HR_CV_REF || cvk == PARC_HR_CV_TAR) {
        const float b = cblend, a = 1.0f - b;
        const float v[4] = {a * cA.x + b * cB.x, a * cA.y + b * cB.y, a * cA.z + b * cB.z, a * cA.w + b * cB.w};
        const int nk = (int)parc_hr_cv_n(hr);
        if (cvk == PARC_HR_CV_REF) { // all four at once: s_refct has 16 slots, and one past the last body has no reader
            const int c = (int)parc_hr_cv_idx(hr);
            *reinterpret_cast<float4 *>(s_refct + 4 * c) = make_float4(v[0], v[1], v[2], v[3]);
            if (MIRROR && P.buf.ref_contacts) {
#pragma unroll
                for (int k = 0; k < 4; ++k) if (k < nk) P.buf.ref_contacts[(size_t)e * B + 4 * c + k] = v[k];
            }
        } else {
            float *o = reinterpret_cast<float *>(reinterpret_cast<char *>(orow) + parc_hr_cv_off(hr));
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < nk) o[k] = v[k];
        }
    } else if (cvk == PARC_HR_CV_VEL) {
        const int c = (int)parc_hr_cv_idx(hr);
        s_refvel[c] = cA;
        if (MIRROR && c == 0 && P.buf.ref_root_vel) { float *o = P.buf.ref_root_vel + 3 * (size_t)e; o[0] = cA.x; o[1] = cA.y; o[2] = cA.z; }
        if (MIRROR && c == 1 && P.buf.ref_root_ang_vel) { float *o = P.buf.ref_root_ang_vel + 3 * (size_t)e; o[0] = cA.x; o[1] = cA.y; o[2] = cA.z; }
        if (MIRROR && c >= 2 && P.buf.ref_dof_vel) {
            const float vv[4] = {cA.x, cA.y, cA.z, cA.w};
            for (int k = 0; k < 4; ++k) { const int d = 4 * (c - 2) + k; if (d < D) P.buf.ref_dof_vel[(size_t)e * D + d] = vv[k]; }
        }
    }
    float bpx = 0.f, bpy = 0.f, bpz = 0.f; // caller-provided rigid-body positions (physics off): in flight during the FK chains
    if (!P.body_pos_from_fk && lane < B) {
        const float *src = P.buf.char_body_pos + 3 * ((size_t)e * B + lane);
        bpx = src[0]; bpy = src[1]; bpz = src[2];
    }
    WAVE_SYNC();
    STAMP(3);

    // ================= FK: row k = lane>>3, root-to-leaf chain c = lane&7 (kin_char_model.py:617-649) =================
    {
        const int k = lane >> 3, c = lane & 7;
        if (k < 2 + S) {
            Q4 prot = s_q[k][0];
            const float4 *jq = k < 2 ? s_lq[k] : s_q[k];
            const float4 pp = s_q[k][15];
            V3 ppos = mk3(pp.x, pp.y, pp.z);
            if (c == 0 && k < 2) {
                s_fk[k * 16] = make_float4(ppos.x, ppos.y, ppos.z, 0.f);
                if (MIRROR && P.tracking) s_br[k][0] = prot;
            }
            int b = s_tab.fk_paths[c][0];
#pragma unroll 1
            for (int d = 0; d < PARC_MAX_FK_DEPTH && b >= 0; ++d) {
                const int nb = d + 1 < PARC_MAX_FK_DEPTH ? s_tab.fk_paths[c][d + 1] : -1; // the chain's next body, known before the product is formed
                const V3 wt = quat_rotate(prot, mk3(s_tab.lt[b][0], s_tab.lt[b][1], s_tab.lt[b][2]));
                ppos = mk3(ppos.x + wt.x, ppos.y + wt.y, ppos.z + wt.z);
                if (nb >= 0 || (MIRROR && P.tracking)) prot = quat_mul(prot, jq[b]); // a leaf's rotation is only read by the tracking-error mirror
                if (k < 2) {
                    s_fk[k * 16 + b] = make_float4(ppos.x, ppos.y, ppos.z, 0.f);
                    if (MIRROR && P.tracking) s_br[k][b] = prot;
                } else {
                    const int slot = s_tab.key_slot[b];
                    if (slot >= 0) s_fk[32 + (k - 2) * 8 + slot] = make_float4(ppos.x, ppos.y, ppos.z, 0.f);
                }
                b = nb;
            }
        }
    }
    WAVE_SYNC();
    if (lane < B) s_cbp[lane] = P.body_pos_from_fk ? s_fk[lane] : make_float4(bpx, bpy, bpz, 0.f);
    STAMP(4);

    // ================= heading pass: every 3-vector of the observation that turns into the heading frame, one per lane =================
    // The targets' root offsets (mgdm_dm_util.py:405-411), the root velocities (ig_char_env.py:593-597) and the key-body offsets of the
    // character and of the targets (ig_char_env.py:603-617, mgdm_dm_util.py:415-440): (source - subtrahend) of the wave's LDS block, rotated by
    // the inverse heading unless the observation is global, to the lane's place in the staged row.  Source, subtrahend and destination are
    // the lane's entry of the table; a target's key offset adds the rotated root offset of its row, which another lane of this pass holds
    // (a lane shuffle; never under global_obs, mgdm_dm_util.py:417).
    if (parc_hr_item(hr)) {
        const char *blk = reinterpret_cast<const char *>(s_q);
        const float *sp = reinterpret_cast<const float *>(blk + parc_hr_src(hr)), *sb = reinterpret_cast<const float *>(blk + parc_hr_sub(hr));
        const V3 rd = mk3(sp[0] - sb[0], sp[1] - sb[1], sp[2] - sb[2]);
        V3 rl = rd;
        if (!GLOBALOBS) {
            rl = quat_rotate(hinv, rd);
            const int a4 = (int)parc_hr_add4(hr); // every lane with an item shuffles (a lane that adds nothing reads lane 0, which has one)
            const float ax = __int_as_float(__builtin_amdgcn_ds_bpermute(a4, __float_as_int(rl.x)));
            const float ay = __int_as_float(__builtin_amdgcn_ds_bpermute(a4, __float_as_int(rl.y)));
            const float az = __int_as_float(__builtin_amdgcn_ds_bpermute(a4, __float_as_int(rl.z)));
            if (parc_hr_adds(hr)) rl = mk3(rl.x + ax, rl.y + ay, rl.z + az);
        }
        float *o = reinterpret_cast<float *>(reinterpret_cast<char *>(s_obs) + parc_hr_dst(hr));
        o[0] = rl.x; o[1] = rl.y; o[2] = rl.z;
    }
    STAMP(5);

    if (MODE == MODE_STEP) {
        // ---- reward + done of the workgroup's four envs on ONE of its waves: 16 lanes per env (row j = env j, lane i of the row = one
        // joint / body / dof / term).  Every sum, exponential and comparison below is one instruction stream for four envs instead of one
        // per env on 1-16 of 64 lanes.  Each wave hands its per-env scalars over through s_sc; the quaternions, FK positions, body
        // positions, reference velocities and contact terms are already in its LDS slice.  The owner rotates with the block index so
        // that the extra work does not pile up on one SIMD.
        {
            float *sc = s_sc_all[wv];
            bool fc = false; // fall rule, first half (mgdm_dm_util.py:349-360): a contact-force component above 0.1 on a non-contact body
            if (P.fall_mask != 0u && lane >= 32 && lane < 32 + B && !((P.fall_mask >> (lane - 32)) & 1u))
                fc = fabsf(aux0) > 0.1f || fabsf(aux1) > 0.1f || fabsf(aux2) > 0.1f;
            const bool fcany = __ballot(fc) != 0ull;
            if (lane == 0) { // (the root velocities are in s_rv since the prefetch phase)
                sc[0] = time; sc[1] = mt; sc[2] = __int_as_float(ts); sc[3] = meta.length; sc[4] = __int_as_float(meta.loop);
                sc[11] = fcany ? 1.f : 0.f; sc[12] = eox; sc[13] = eoy; sc[14] = __int_as_float(e);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // the four waves' LDS slices are complete (waves of a short last block have left)
        const int nact = min(ENVS_PER_BLOCK, count - (int)blockIdx.x * ENVS_PER_BLOCK);
        int owner = blockIdx.x & (ENVS_PER_BLOCK - 1);
        if (owner >= nact) owner = 0;
        if (wv == owner) {
            const int j = lane >> 4, i = lane & 15, rowbase = lane & 48;
            const bool valid = j < nact;
            const int jj = valid ? j : 0;
            const float4 (*q)[16] = reinterpret_cast<const float4 (*)[16]>(s_blk_all[jj] + PARC_HROT_Q_F4);
            const float4 *fk = s_blk_all[jj] + PARC_HROT_FK_F4;
            const float4 *cbp = s_lq_all[jj][0];
            const float *scj = s_sc_all[jj];
            const float4 rp4 = q[0][15], trp = q[1][15];
            // reward terms, one per lane (mgdm_dm_util.py:270-333, 498-518); every row sum is taken at the row's lane 0
            float dang = 0.f, vpose = 0.f;
            Q4 hinv_c = mk4(0.f, 0.f, 0.f, 1.f), hinv_r = hinv_c; // LOCALROOT: inverse heading of the character / of the reference
            if (LOCALROOT) {
                hinv_c = heading_quat_inv(calc_heading(q[0][0]));
                hinv_r = heading_quat_inv(calc_heading(q[1][0]));
            }
            if (i <= J) { // angle of ref (x) conj(char): joints on lanes < J, the root on lane J (slot 0 of both rows)
                const int slot = i < J ? 1 + i : 0;
                if (LOCALROOT) {
                    Q4 qa = q[0][slot], qb = q[1][slot];
                    if (i == J) { qa = quat_mul(hinv_c, qa); qb = quat_mul(hinv_r, qb); }
                    dang = quat_diff_angle(qa, qb);
                } else {
                    dang = quat_diff_angle(q[0][slot], q[1][slot]);
                }
                if (i < J) vpose = T->joint_err_w[i] * dang * dang;
            }
            float vs[4] = {0.f, 0.f, 0.f, 0.f}; // dof velocity terms, 16 dofs per pass (the sums pair up as the four 16-lane rows of a wave would)
#pragma unroll
            for (int pss = 0; pss < (PARC_MAX_DOFS + 15) / 16; ++pss) {
                if (16 * pss < D) { // uniform
                    const int d = 16 * pss + i;
                    float v = 0.f;
                    if (d < D) {
                        const float dv = ((const float *)s_refvel_all[jj])[8 + d] - s_cdofv_all[jj][d];
                        v = T->dof_err_w[d] * dv * dv;
                    }
                    vs[pss] = row_sum16(v);
                }
            }
            float vkey = 0.f;
            if (i < K) { // key positions: simulator bodies vs reference FK (ig_parkour_env.py:987)
                const int b = s_tab.key_ids[i];
                const float4 kp = cbp[b], tk = fk[16 + b];
                if (LOCALROOT) {
                    const V3 kt = quat_rotate(hinv_r, mk3(tk.x - trp.x, tk.y - trp.y, tk.z - trp.z));
                    const V3 kc = quat_rotate(hinv_c, mk3(kp.x - rp4.x, kp.y - rp4.y, kp.z - rp4.z));
                    const float dx = kt.x - kc.x, dy = kt.y - kc.y, dz = kt.z - kc.z;
                    vkey = dx * dx + dy * dy + dz * dz;
                } else {
                    const float dx = (tk.x - trp.x) - (kp.x - rp4.x);
                    const float dy = (tk.y - trp.y) - (kp.y - rp4.y);
                    const float dz = (tk.z - trp.z) - (kp.z - rp4.z);
                    vkey = dx * dx + dy * dy + dz * dz;
                }
            }
            float vct = 0.f;
            if (i < B) { // contact term
                const float tar = s_refct_all[jj][i], f = s_cfn_all[jj][i];
                float cr = -(1.0f - tar) * f;
                cr = cr + tar * f;
                vct = T->contact_w[i] * cr;
            }
            // ---- early termination (mgdm_dm_util.py:335-402) ----
            bool bad = false;
            if (i >= 1 && i < B) {
                const float4 bp = cbp[i], b0 = cbp[0], tp = fk[16 + i], t0 = fk[16];
                const float dx = (tp.x - t0.x) - (bp.x - b0.x);
                const float dy = (tp.y - t0.y) - (bp.y - b0.y);
                const float dz = (tp.z - t0.z) - (bp.z - b0.z);
                const float lim = T->pose_term_dist[i - 1];
                bad = (dx * dx + dy * dy + dz * dz) > lim * lim;
            }
            const bool pose_fail_any = ((unsigned)(__ballot(bad) >> rowbase) & 0xffffu) != 0u;
            // fall rule, second half: a non-contact body lower than termination_height above the terrain under it (global xy = env-local
            // + env offset, :147-152)
            bool fallen = false;
            if (P.fall_mask != 0u) { // uniform
                bool fh = false;
                if (i < B && !((P.fall_mask >> i) & 1u)) {
                    const float4 bp = cbp[i];
                    const int ix = min(max(cell_index(bp.x + scj[12], P.min_x, P.dx), 0), P.X - 1), iy = min(max(cell_index(bp.y + scj[13], P.min_y, P.dy), 0), P.Y - 1);
                    fh = bp.z < P.hf[(size_t)ix * P.Y + iy] + P.term_h;
                }
                fallen = scj[11] != 0.f && ((unsigned)(__ballot(fh) >> rowbase) & 0xffffu) != 0u;
            }
            const float root_rot_angle = __shfl(dang, rowbase + J, 64);
            const float pose_err = __shfl(row_sum16(vpose), rowbase, 64), csum = __shfl(row_sum16(vct), rowbase, 64), key_err = __shfl(row_sum16(vkey), rowbase, 64);
            const float vel_err = __shfl((vs[0] + vs[1]) + (vs[2] + vs[3]), rowbase, 64);

            // per-env tail: every lane of a row carries its env's values; the five exponentials run on lanes 0..4 of the row
            const float time_j = scj[0], mt_j = scj[1], mlen_j = scj[3];
            const int ts_j = __float_as_int(scj[2]), mloop_j = __float_as_int(scj[4]), e_j = __float_as_int(scj[14]);
            float rdx = trp.x - rp4.x, rdy = trp.y - rp4.y, rdz = trp.z - rp4.z;
            if (!P.track_root) { rdx = 0.f; rdy = 0.f; }
            if (!P.track_root_h) rdz = 0.f;
            const float root_pos_err = rdx * rdx + rdy * rdy + rdz * rdz;
            const float4 tv = s_refvel_all[jj][0], tav = s_refvel_all[jj][1];
            const float4 cv = s_blk_all[jj][PARC_HROT_RV_F4 + 0], cav = s_blk_all[jj][PARC_HROT_RV_F4 + 1]; // the character's root velocities
            const float rre = root_rot_angle * root_rot_angle;
            float rve, rave;
            if (LOCALROOT) {
                const V3 tv3 = quat_rotate(hinv_r, mk3(tv.x, tv.y, tv.z)), tav3 = quat_rotate(hinv_r, mk3(tav.x, tav.y, tav.z));
                const V3 rv3 = quat_rotate(hinv_c, mk3(cv.x, cv.y, cv.z)), rav3 = quat_rotate(hinv_c, mk3(cav.x, cav.y, cav.z));
                float d0 = tv3.x - rv3.x, d1 = tv3.y - rv3.y, d2 = tv3.z - rv3.z;
                rve = d0 * d0 + d1 * d1 + d2 * d2;
                d0 = tav3.x - rav3.x; d1 = tav3.y - rav3.y; d2 = tav3.z - rav3.z;
                rave = d0 * d0 + d1 * d1 + d2 * d2;
            } else {
                float d0 = tv.x - cv.x, d1 = tv.y - cv.y, d2 = tv.z - cv.z;
                rve = d0 * d0 + d1 * d1 + d2 * d2;
                d0 = tav.x - cav.x; d1 = tav.y - cav.y; d2 = tav.z - cav.z;
                rave = d0 * d0 + d1 * d1 + d2 * d2;
            }
            float earg = -0.25f * pose_err;
            earg = i == 1 ? -0.01f * vel_err : earg;
            earg = i == 2 ? -5.0f * (root_pos_err + 0.1f * rre) : earg;
            earg = i == 3 ? -1.0f * (rve + 0.1f * rave) : earg;
            earg = i == 4 ? -10.0f * key_err : earg;
            const float eval = expf(earg);
            const float pose_r = __shfl(eval, rowbase, 64), vel_r = __shfl(eval, rowbase + 1, 64), root_pose_r = __shfl(eval, rowbase + 2, 64),
                        root_vel_r = __shfl(eval, rowbase + 3, 64), key_pos_r = __shfl(eval, rowbase + 4, 64);
            float rew = P.pose_w * pose_r + P.vel_w * vel_r + P.root_pos_w * root_pose_r + P.root_vel_w * root_vel_r + P.key_pos_w * key_pos_r;
            const float contact_pen = (OBSVAR && P.obs_contact == 0) ? 0.f : csum / (float)B; // torch.mean over bodies (ig_parkour_env.py:1033); no term without use_contact_info (:1032)
            rew = rew + contact_pen;
            // done (compute_done + DeepMimicEnv.update_done dm_env.py:628-665)
            int done = PARC_DONE_NULL;
            if (time_j >= P.episode_length) done = PARC_DONE_TIME;
            if (P.early_term) {
                bool failed = fallen;
                if (P.pose_term) {
                    bool pf = pose_fail_any;
                    if (P.track_root) {
                        const float4 b0 = cbp[0], t0 = fk[16];
                        const float ex = b0.x - t0.x, ey = b0.y - t0.y, ez = b0.z - t0.z;
                        pf = pf || (ex * ex + ey * ey + ez * ez) > P.root_pos_term_sq;
                        pf = pf || fabsf(root_rot_angle) > P.root_rot_term;
                    }
                    failed = failed || pf;
                }
                if (!(time_j > 1e-5f)) failed = false;
                if (failed) done = PARC_DONE_FAIL;
            }
            const bool motion_end = (mt_j >= mlen_j) && (mloop_j != PARC_LOOP_WRAP);
            unsigned char code = 0;
            if (done != PARC_DONE_NULL || motion_end) code = (done == PARC_DONE_FAIL) ? 1 : 2;
            if (motion_end) done = PARC_DONE_FAIL;
            if (P.never_done) done = PARC_DONE_NULL; // ig_parkour_env.py:980: after update_done (the curriculum still sees the episode end)
            if (valid && i == 0) {
                P.buf.reward[e_j] = rew;
                P.buf.done[e_j] = done;
                P.ema_code[e_j] = code;
                P.buf.timestep[e_j] = ts_j;
                if (P.buf.time) P.buf.time[e_j] = time_j;
            }
            if (P.buf.reward_terms && valid && i < 7) {
                const float vals[7] = {pose_r, vel_r, root_pose_r, root_vel_r, key_pos_r, contact_pen, rew};
                float v = vals[0];
#pragma unroll
                for (int qq = 1; qq < 7; ++qq) v = i == qq ? vals[qq] : v;
                P.buf.reward_terms[(size_t)i * P.N + e_j] = v;
            }
        }

        // optional outputs: ref body positions / dof positions, tracking error
        if (MIRROR && P.buf.ref_body_pos && lane < B) {
            float *o = P.buf.ref_body_pos + 3 * ((size_t)e * B + lane);
            const float4 v = s_fk[16 + lane];
            o[0] = v.x; o[1] = v.y; o[2] = v.z;
        }
        if (MIRROR && P.buf.ref_dof_pos && lane >= 1 && lane < B) { // kin_char_model.py:601
            const int ty = T->h.jtype[lane];
            float out3[3] = {0.f, 0.f, 0.f};
            joint_rot_to_dof(ty, T->h.axis[lane], s_q[1][lane], out3);
            const int nd = ty == PARC_JOINT_HINGE ? 1 : (ty == PARC_JOINT_SPHERICAL ? 3 : 0);
            for (int k = 0; k < nd; ++k) P.buf.ref_dof_pos[(size_t)e * D + T->h.dof_idx[lane] + k] = out3[k];
        }
        if (MIRROR && P.tracking && P.buf.tracking_error) { // mgdm_dm_util.py:521-553 (per wave: an optional output, off in training)
            const float4 trp = s_q[1][15], tv = s_refvel[0], tav = s_refvel[1];
            const float root_rot_angle = quat_diff_angle(s_q[0][0], s_q[1][0]);
            const float rvx = lane_value(aux0, 30), rvy = lane_value(aux1, 30), rvz = lane_value(aux2, 30);
            const float rax = lane_value(aux0, 31), ray_ = lane_value(aux1, 31), raz = lane_value(aux2, 31);
            float e_rot = 0.f, e_pos = 0.f, e_dv = 0.f;
            if (lane < B) {
                e_rot = fabsf(quat_diff_angle(s_br[0][lane], s_br[1][lane]));
                const float4 cb = s_fk[lane], rb = s_fk[16 + lane];
                e_pos = norm3(mk3((rb.x - trp.x) - (cb.x - root_pos.x), (rb.y - trp.y) - (cb.y - root_pos.y), (rb.z - trp.z) - (cb.z - root_pos.z)));
            }
            if (lane < D) e_dv = fabsf(((const float *)s_refvel)[8 + lane] - s_cdofv[lane]);
            const float pe = wave_sum(e_rot), bpe = wave_sum(e_pos), dve = wave_sum(e_dv);
            if (lane == 0) {
                float *te = P.buf.tracking_error + 7 * (size_t)e;
                te[0] = norm3(mk3(trp.x - root_pos.x, trp.y - root_pos.y, trp.z - root_pos.z));
                te[1] = fabsf(root_rot_angle);
                te[2] = bpe / (float)B;
                te[3] = pe / (float)B;
                te[4] = dve / (float)D;
                te[5] = (fabsf(tv.x - rvx) + fabsf(tv.y - rvy) + fabsf(tv.z - rvz)) / 3.f;
                te[6] = (fabsf(tav.x - rax) + fabsf(tav.y - ray_) + fabsf(tav.z - raz)) / 3.f;
            }
        }
    }
    if (P.body_pos_from_fk && P.buf.char_body_pos && lane < B) {
        float *o = P.buf.char_body_pos + 3 * ((size_t)e * B + lane);
        const float4 v = s_fk[lane];
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    }
    WAVE_SYNC();
    STAMP(6);

    // ================= stream the staged observation prefix out: 16 bytes per lane per store =================
    {
        const int nst = P.off_tarc; // [0, off_tarc) staged; contacts and rays were stored directly
        if ((P.obs_dim & 3) == 0) {
            const float4 *src = (const float4 *)s_obs;
            float4 *dst = (float4 *)orow;
            const int n4 = nst >> 2;
            for (int i = lane; i < n4; i += 64) dst[i] = src[i];
            for (int i = 4 * n4 + lane; i < nst; i += 64) orow[i] = s_obs[i];
        } else {
            for (int i = lane; i < nst; i += 64) orow[i] = s_obs[i];
        }
    }
    STAMP(7);
#ifdef PARC_STAMPS
    WAVE_SYNC();
    if (lane < 7 && P.stamp_out) P.stamp_out[(size_t)e * 8 + lane] = (unsigned)(s_stamp[lane + 1] - s_stamp[lane]);
    if (lane == 7 && P.stamp_out) P.stamp_out[(size_t)e * 8 + 7] = 0;
#endif
}
