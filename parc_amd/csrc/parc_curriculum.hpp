// parc_curriculum.hpp — the kernels that close a step: the ordered list of finished envs (k_done_scatter), the fail-rate EMA of the
// curriculum over it on its three paths (k_curriculum_small; k_fail_rate_ema; k_ema_first + k_ema_leader), and the dynamics' health words.
#pragma once
#include <hip/hip_runtime.h>

#include "parc_dynamics_host.hpp"   // ParcDynCounters
#include "parc_env_tables.hpp"      // wave_scan_incl, wave_totals

// ------------------------------------------------------------------------------------------------
// curriculum: sequential fail-rate EMA in env order (dm_env.py:646-660), exact op order per motion.
//   k_done_scatter: ordered (stable) compaction of the finished envs, one block per 1024 envs; the per-chunk
//                   totals were counted by the step kernel, so a block's base offset is a 128-term sum.
//   k_fail_rate_ema: one wave per motion walks the env-ordered list 64 entries at a time and applies
//                   f <- f*(1-w)+w (FAIL) / f <- f*(1-w) (TIME, SUCC, motion end) in that order.
// The compacted list doubles as the env-id list of parc_env_reset_done (no nonzero(), no host sync).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int nonzero_bytes(unsigned v) {
    return ((v & 0xffu) != 0) + ((v & 0xff00u) != 0) + ((v & 0xff0000u) != 0) + ((v & 0xff000000u) != 0);
}

// Block b owns envs [1024 b, 1024 b + 1024).  Its base offset = number of finished envs before it, which it
// counts itself from the (1 byte per env) code array: no atomics in the step kernel, no second launch.
__device__ __forceinline__ void done_scatter_block(const unsigned char *__restrict__ ema_code, const int *__restrict__ motion_ids, int N, int *done_list,
                                                   int *done_key, int *reset_count, int never_done, int b, int nblocks) {
    __shared__ int s_base, s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    {
        const uint4 *src = (const uint4 *)ema_code; // hipMalloc'd: 16-byte aligned; 1024 b bytes = 64 b uint4
        int c = 0;
        for (int i = tid; i < 64 * b; i += 1024) {
            const uint4 v = src[i];
            c += nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
        }
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == 0 && c) atomicAdd(&s_base, c);
    }
    const int e = b * 1024 + tid;
    const unsigned char code = e < N ? ema_code[e] : 0;
    const unsigned long long mask = __ballot(code != 0);
    const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(mask);
    __syncthreads();
    const WaveTotals wt = wave_totals(s_wave, wv);
    const int woff = wt.woff, total = wt.total;
    if (code) {
        const int pos = s_base + woff + prefix;
        done_list[pos] = e;
        done_key[pos] = (motion_ids[e] << 1) | (code == 1 ? 1 : 0);
    }
    if (b == nblocks - 1 && tid == 0) {
        reset_count[0] = s_base + total;                   // entries of the list: the fail-rate EMA walks all of them
        reset_count[1] = never_done ? 0 : s_base + total;  // envs parc_env_reset_done resets (never_done: flags are NULL, nobody)
    }
}
// The health counters of the dynamics kernel (flag waits that timed out, contact planes that found no slot) go to two words of
// host-mapped pinned memory with the first launch after every step: the host reads them without a synchronisation or a copy
// (HipParkourEnv.step looks at them every step: a protocol error aborts the run at the next step instead of at the next log interval).
// `words` is null when there is nothing to publish (no dynamics, or no mapped memory): the host's words then stay 0.
struct HealthOut {
    unsigned int *words;     // device alias of the host's two words
    ParcDynCounters from;    // the counters of the dynamics unit
};
__device__ __forceinline__ void publish_health(const HealthOut &health) {
    if (health.words && blockIdx.x == 0 && threadIdx.x == 0) {
        __builtin_nontemporal_store(*health.from.timeouts, health.words);
        __builtin_nontemporal_store(*health.from.man_drops, health.words + 1);
    }
}

__global__ __launch_bounds__(1024) void k_done_scatter(const unsigned char *__restrict__ ema_code, const int *__restrict__ motion_ids,
                                                       int N, int *done_list, int *done_key, int *reset_count, int never_done, HealthOut health) {
    publish_health(health);
    done_scatter_block(ema_code, motion_ids, N, done_list, done_key, reset_count, never_done, blockIdx.x, gridDim.x);
}

// One 1024-thread block per motion.  The block sweeps the env-ordered list and compacts (stable, by rank) the addends of its
// motion's entries -- w for FAIL, +0 otherwise -- into LDS; thread 0 then applies the chain in that order:
// f <- f*(1-w) + addend  (adding +0.0f leaves f*(1-w) unchanged, so this is the reference's two-branch update,
// dm_env.py:651-658, bit for bit).  The chain is inherently serial (each update rounds): only its two dependent VALU
// operations per entry stay on it, the addends arrive four at a time from LDS.
#define EMA_CAP 8192
// the chain itself, on one thread: f <- f*keep + addend over `n` buffered addends (eight LDS reads in flight: only the first one's latency is exposed)
__device__ __forceinline__ float ema_chain(float f, const float *s_add, int n, float keep) {
    int i4 = 0;
    const float4 *a4 = (const float4 *)s_add;
    for (; i4 + 32 <= n; i4 += 32) {
        float4 q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = a4[(i4 >> 2) + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f = f * keep; f = f + q[j].x;
            f = f * keep; f = f + q[j].y;
            f = f * keep; f = f + q[j].z;
            f = f * keep; f = f + q[j].w;
        }
    }
    for (; i4 + 4 <= n; i4 += 4) {
        const float4 a = a4[i4 >> 2];
        f = f * keep; f = f + a.x;
        f = f * keep; f = f + a.y;
        f = f * keep; f = f + a.z;
        f = f * keep; f = f + a.w;
    }
    for (; i4 < n; ++i4) { f = f * keep; f = f + s_add[i4]; }
    return f;
}
// Where the eight (match, fail) bits a thread contributes to a pass come from: n() entries to sweep in env order, bits(e0, m, ..) = those of
// entries e0 .. e0 + 7 for motion m (e0 a multiple of 8).
// The compacted, env-ordered key list ((motion << 1) | fail bit): two 16-byte loads per thread, single loads on the ragged tail.
// (Round 3: the list was swept 1 024 entries at a time with two barriers per sweep -- 1.5 us per sweep, six sweeps per step at 65 536 envs.)
struct EmaKeyList {
    const int *__restrict__ done_key;
    int k;
    __device__ __forceinline__ int n() const { return k; }
    __device__ __forceinline__ void bits(int e0, int m, unsigned &matchbits, unsigned &failbits) const {
        int key[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) key[j] = -2;
        if (e0 + 8 <= k) { // the list buffer is 16-byte aligned and e0 a multiple of 8
            const int4 a = *(const int4 *)(done_key + e0), c = *(const int4 *)(done_key + e0 + 4);
            key[0] = a.x; key[1] = a.y; key[2] = a.z; key[3] = a.w; key[4] = c.x; key[5] = c.y; key[6] = c.z; key[7] = c.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (e0 + j < k) key[j] = done_key[e0 + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (key[j] >= 0 && (key[j] >> 1) == m) { matchbits |= 1u << j; if (key[j] & 1) failbits |= 1u << j; }
    }
};
// The step kernel's per-env codes (1 byte per env: 0 = not finished, 1 = FAIL, 2 = other), for shards of up to CURRICULUM_ONE_LAUNCH_MAX
// envs: one 8-byte load per thread; finished envs are few, so their motion ids are conditional loads.
struct EmaEnvCodes {
    const unsigned char *__restrict__ ema_code;
    const int *__restrict__ motion_ids;
    int N; // a multiple of 8 on this path (curriculum_path)
    __device__ __forceinline__ int n() const { return N; }
    __device__ __forceinline__ void bits(int e0, int m, unsigned &matchbits, unsigned &failbits) const {
        unsigned long long codes = 0ull;
        if (e0 < N) codes = *(const unsigned long long *)(ema_code + e0);
        if (codes) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned c = (unsigned)(codes >> (8 * j)) & 0xffu;
                if (c && motion_ids[e0 + j] == m) { matchbits |= 1u << j; if (c == 1u) failbits |= 1u << j; }
            }
        }
    }
};
// One pass per EMA_CAP entries of the source: every thread takes 8 consecutive entries, a block-wide exclusive scan of the per-thread match
// counts places the motion's addends in env order, thread 0 runs the chain.
template <class Source>
__device__ __forceinline__ void fail_rate_ema_block(const Source &src, float *fail_rates, int m, float w) {
    __shared__ __align__(16) float s_add[EMA_CAP];
    __shared__ int s_wtot[16];
    __shared__ float s_f;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float keep = (float)(1.0 - (double)w);
    if (tid == 0) s_f = fail_rates[m];
    bool any = false;
    for (int base = 0; base < src.n(); base += EMA_CAP) {
        unsigned matchbits = 0u, failbits = 0u;
        src.bits(base + 8 * tid, m, matchbits, failbits);
        const int cnt = __popc(matchbits);
        const int incl = wave_scan_incl(cnt, lane);
        __syncthreads(); // s_f / the previous pass's buffer are settled
        if (lane == 63) s_wtot[wv] = incl;
        __syncthreads();
        const WaveTotals wt = wave_totals(s_wtot, wv);
        const int total = wt.total;
        int pos = wt.woff + incl - cnt;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (matchbits & (1u << j)) s_add[pos++] = (failbits & (1u << j)) ? w : 0.0f;
        __syncthreads();
        if (total > 0) { // uniform
            any = true;
            if (tid == 0) s_f = ema_chain(s_f, s_add, total, keep);
        }
    }
    __syncthreads();
    if (tid == 0 && any) fail_rates[m] = s_f;
}
__global__ __launch_bounds__(1024) void k_fail_rate_ema(const int *__restrict__ done_key, const int *__restrict__ reset_count,
                                                       float *fail_rates, int M, float w) {
    const int k = *reset_count, m = blockIdx.x;
    if (k == 0 || m >= M) return;
    fail_rate_ema_block(EmaKeyList{done_key, k}, fail_rates, m, w);
}
// Both of the above as ONE launch, for shards of up to CURRICULUM_ONE_LAUNCH_MAX envs (what a GPU of an 8-GPU job runs): blocks [0, nchunks) compact the finished envs
// (the reset list), blocks nchunks.. apply the EMA of motion m -- reading the step kernel's per-env codes directly instead of the compacted
// list, so that no block waits for another.  Same entries in the same (env) order: bit-identical to the two launches.
#define CURRICULUM_ONE_LAUNCH_MAX 8192 // measured: -1.6 us per step at 8 192 envs, +1.6 us at 16 384 (two passes of the scan)
__global__ __launch_bounds__(1024) void k_curriculum_small(const unsigned char *__restrict__ ema_code, const int *__restrict__ motion_ids, int N,
                                                          int *done_list, int *done_key, int *reset_count, int never_done, int nchunks,
                                                          float *fail_rates, int M, float w, HealthOut health) {
    publish_health(health);
    if ((int)blockIdx.x < nchunks) {
        done_scatter_block(ema_code, motion_ids, N, done_list, done_key, reset_count, never_done, blockIdx.x, nchunks);
    } else {
        const int m = (int)blockIdx.x - nchunks;
        if (m >= M) return;
        fail_rate_ema_block(EmaEnvCodes{ema_code, motion_ids, N}, fail_rates, m, w);
    }
}

// Large libraries (thousands of motions, a handful of finished envs each): one block per motion sweeping the whole list is
// O(M k).  Instead the FIRST list entry of every motion that occurs becomes its leader (atomicMin over a per-motion slot
// that is kept at INT_MAX between steps), and the leader walks the list once, applying its motion's entries in list
// (= env) order: the same chain, the same roundings, O(k) per motion that actually finished an env.
__global__ void k_ema_first(const int *__restrict__ done_key, const int *__restrict__ reset_count, int *first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *reset_count) return;
    atomicMin(&first[done_key[i] >> 1], i);
}

__global__ __launch_bounds__(256) void k_ema_leader(const int *__restrict__ done_key, const int *__restrict__ reset_count, int *first,
                                                    float *fail_rates, float w) {
    // one WAVE per list entry; only the waves of leaders do anything.  The 64 lanes sweep the rest of the list 64 entries at
    // a time (one coalesced load, two ballots); lane 0 applies the matching entries of a tile in list order.
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const int k = *reset_count;
    if (i >= k) return;
    const int m = done_key[i] >> 1;
    if (first[m] != i) return;
    const float keep = (float)(1.0 - (double)w);
    float f = fail_rates[m];
    for (int j0 = i & ~63; j0 < k; j0 += 64) {
        const int j = j0 + lane;
        const int key = j < k ? done_key[j] : -2;
        const bool match = j >= i && (key >> 1) == m;
        unsigned long long mm = __ballot(match);
        const unsigned long long ff = __ballot(match && (key & 1));
        while (mm) { // uniform: every lane runs the same chain, lane 0 stores
            const int t = __builtin_ctzll(mm);
            mm &= mm - 1ull;
            f = f * keep;
            f = f + (((ff >> t) & 1ull) ? w : 0.0f);
        }
    }
    if (lane == 0) { fail_rates[m] = f; first[m] = 0x7fffffff; }
}
