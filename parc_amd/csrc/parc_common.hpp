// parc_common.hpp — what more than one of the library's units (parc_env.hip, parc_dynamics.hip, parc_tools.hip) uses, and nothing else.
//   host:   the thread's last error message (one instance for the whole library), fail / HIPCHK / PARC_TRY, blocks, the device arena, the event set,
//           dev_opt
//   device: Philox4x32-10 and the frame blend of motion_lib.py (the motion table entry it reads: parc_motion_table.hpp)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_motion_table.hpp"   // MotionMeta, and the host code that fills it

// ================================================================================================
// host side
// ================================================================================================
inline thread_local std::string g_err;   // parc_last_error() (parc_env.hip) returns it
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(PARC_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

#define PARC_TRY(x) do { if (int _rc = (x)) return _rc; } while (0)

static unsigned blocks(long long n, int t) { return (unsigned)((n + t - 1) / t); }

// ParcEnvConfig::dev_options, "key=value;key=value"
static std::string dev_opt(const ParcEnvConfig *cfg, const char *key) {
    if (!cfg->dev_options) return "";
    const std::string all = cfg->dev_options, k = std::string(key) + "=";
    size_t at = 0;
    while (at < all.size()) {
        size_t end = all.find(';', at);
        if (end == std::string::npos) end = all.size();
        if (all.compare(at, k.size(), k) == 0) return all.substr(at + k.size(), end - at - k.size());
        at = end + 1;
    }
    return "";
}

struct DeviceArena {                      // device buffers with one lifetime: freed together, by release() or with the arena
    std::vector<void *> ptrs;
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { release(); }
    // p = count elements of T on the current device (16 B when count is 0), copied from the host array src when given
    template <typename T> int alloc(T *&p, long long count, const void *src = nullptr) {
        void *d = nullptr;
        const size_t bytes = count > 0 ? (size_t)count * sizeof(T) : 16;
        HIPCHK(hipMalloc(&d, bytes));
        ptrs.push_back(d);
        if (src && count > 0) HIPCHK(hipMemcpy(d, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
        p = (T *)d;
        return PARC_OK;
    }
    // p = count elements of T, every byte set to `byte`
    template <typename T> int alloc_fill(T *&p, long long count, int byte = 0) {
        PARC_TRY(alloc(p, count));
        if (count > 0) HIPCHK(hipMemset(p, byte, (size_t)count * sizeof(T)));
        return PARC_OK;
    }
    void swap(DeviceArena &o) { ptrs.swap(o.ptrs); }
    void release() {
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

template <int N> struct DeviceEvents {    // N events with one lifetime, indexed like the array they are: ev[i]
    hipEvent_t ev[N] = {};
    DeviceEvents() = default;
    DeviceEvents(const DeviceEvents &) = delete;
    DeviceEvents &operator=(const DeviceEvents &) = delete;
    ~DeviceEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    int create() {                        // on the current device, once
        for (hipEvent_t &e : ev) HIPCHK(hipEventCreate(&e));
        return PARC_OK;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
    int elapsed(float &ms, int from, int to) const {   // ms between two recorded events
        HIPCHK(hipEventElapsedTime(&ms, ev[from], ev[to]));
        return PARC_OK;
    }
};

// ================================================================================================
// device side
// ================================================================================================
struct Blend { int i0, i1; float b; };

// motion_lib.py:425-438 (+ calc_phase :520)
__device__ __forceinline__ Blend frame_blend(const MotionMeta &m, float t) {
    float phase = t / m.length;
    if (m.loop == PARC_LOOP_WRAP) phase = phase - floorf(phase);
    phase = fminf(fmaxf(phase, 0.f), 1.f);
    float pf = phase * (float)(m.nframes - 1);
    int f0 = (int)pf;                       // .long(): truncation
    f0 = max(0, min(f0, m.nframes - 1));    // memory safety only (no-op for finite phase)
    int f1 = min(f0 + 1, m.nframes - 1);
    Blend r;
    r.b = pf - (float)f0;
    r.i0 = f0 + m.start;
    r.i1 = f1 + m.start;
    return r;
}

// ---- device RNG: Philox4x32-10 -------------------------------------------------------------------
__device__ __forceinline__ void philox_round(unsigned &c0, unsigned &c1, unsigned &c2, unsigned &c3, unsigned k0, unsigned k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
__device__ __forceinline__ void philox4(unsigned long long seed, unsigned long long ctr_hi, unsigned ctr_lo, float *u4) {
    unsigned c0 = ctr_lo, c1 = (unsigned)ctr_hi, c2 = (unsigned)(ctr_hi >> 32), c3 = 0x5041524Bu;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    for (int r = 0; r < 10; ++r) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    u4[0] = (c0 >> 8) * (1.0f / 16777216.0f); u4[1] = (c1 >> 8) * (1.0f / 16777216.0f);
    u4[2] = (c2 >> 8) * (1.0f / 16777216.0f); u4[3] = (c3 >> 8) * (1.0f / 16777216.0f);
}
