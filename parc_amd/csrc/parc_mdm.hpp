// parc_mdm.hpp — the motion generator's inference on gfx950 (parc_mdm_*, include/parc_env.h): the reference's MDMTransformer
// (motion_generator/mdm_transformer.py) in eval mode and fp32, and the reverse-diffusion loops of motion_generator/mdm.py.
//   k_mdm_cond     embed_conds, once per generation: the 31 x 31 tokenizer (three 5 x 5 convolutions and one 4 x 4, LeakyReLU, Unfold(2, 2)),
//                  _obs_embed, the target MLP, the flags of the batch (and x_T when it is drawn on the device)
//   k_mdm_forward  one pass: one workgroup of 4 waves owns one sample from its tokens to x_0.  The residual stream stays in LDS; Q/K/V,
//                  the attention output and the hidden layers go through a scratch buffer in global memory indexed by the workgroup (the grid
//                  is the number of resident workgroups, so the scratch stays in L2); the weights stream from L2.  With guidance both passes
//                  of a step are rows of one launch.
//   k_mdm_update   lane per frame: the guidance combine, project_dofs (un-standardise, exp map / dofs -> quaternions, FK, back, standardise)
//                  and the DDIM or DDPM step
// Every product of the network goes through mma16, the one MFMA micro-tile (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation
// in k order).  No atomics, no reduction across samples: a sample's bits do not depend on its batch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_math.hpp"
#include "parc_char.hpp"
#include "parc_tool_handle.hpp"

namespace mdm {
using namespace parc;

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WG = 256, NW = 4;            // k_mdm_forward / k_mdm_cond: 4 waves, one per SIMD
constexpr int MAXMT = 9;                   // row tiles of 16: 1 + 64 + 1 + 1 + 64 tokens = 131 -> 144
constexpr int NCOND = 65;                  // cached condition tokens: 64 heightfield tokens, the target token
constexpr int NC = 67;                     // tokens before the motion frames: time, 64 heightfield, target, indicator
constexpr int TOK_DIM = 256;               // 64 channels x 2 x 2 of the tokenizer
constexpr int CONV_A = 32 * 27 * 27, CONV_B = 32 * 23 * 23;   // the two largest activations of the tokenizer
constexpr int UPD_T = 64;                  // k_mdm_update: frames per block
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2 };
enum { F_OBS = 1, F_TARGET = 2, F_PREV = 4, F_IND = 8 };

struct Lin { const float *w, *b; int N, K, Np, Kp; };   // a Linear, rows and columns zero-padded to multiples of 16: w [Np][Kp], b [Np]
struct Layer { Lin qkv, out, l1, l2; const float *n1w, *n1b, *n2w, *n2b; };
struct Net {                               // device memory, read with uniform indices
    int d, H, hd, dh, L, T, nprev, D, DP, TP, NP, NPAD, MT, xrows, ldx, lds, timesteps;
    long long r1, r2;                      // floats of the two scratch regions of a slot
    const float *conv_w[4], *conv_b[4];
    Lin obs, time0, time1;
    int ntgt, nin, nout;
    Lin tgt[PARC_MDM_MAX_HIDDEN + 1], inm[PARC_MDM_MAX_HIDDEN + 1], outm[PARC_MDM_MAX_HIDDEN + 1];
    const float *ind_embed, *pe_time, *pe_seq, *mean, *std;
    Layer layer[PARC_MDM_MAX_LAYERS];
};
struct Batch {                             // the handle's cache of one embed_conds, by value
    int n;
    float *tokens;                         // [n][NCOND][d]
    float *prev;                           // [n][nprev][D]
    int *flags;                            // [n] F_*
    float *scratch;                        // [slots][r1 + r2]
};

// ---- the GEMM micro-tile ------------------------------------------------------------------------------------------------------------
// acc [16 x 16] += A [16 x 16] B [16 x 16] for one chunk of 16 along k.  Lane l holds row (of A) / column (of B) l & 15 and the four k
// 4 g .. 4 g + 3 of its group g = l >> 4: a = A[l & 15][4 g ..], b = B[4 g ..][l & 15].  MFMA s sums k = 4 g + s over the four groups.
// acc: column l & 15, rows 4 g + r.  A bf16-operand mode replaces this function (and the loads that feed it) only.
__device__ __forceinline__ f32x4 mma16(float4 a, float4 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
    return c;
}

__device__ __forceinline__ float act(int a, float v) {
    if (a == ACT_SILU) return v / (1.f + expf(-v));
    if (a == ACT_GELU) return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
    return v;
}

// out[m][n] = act(sum_k A[m][k] W[n][k] + b[n]) * oscale (+ res[m][n]) for mt row tiles of 16 and every column tile of W, stored for
// m < m_valid, n < n_valid.  A, out and res may be LDS or global; A has Kp readable columns (lda a multiple of 4 floats, 16-byte aligned)
// and 16 mt readable rows; res shares out's leading dimension (out may be res).  A wave owns whole column tiles: it reads each weight once.
template <int ACT>
__device__ __forceinline__ void gemm(const float *A, int lda, int mt, const Lin &W, float *out, int ldo, int m_valid, int n_valid, const float *res,
                                     float oscale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const int Kp = W.Kp, ntn = W.Np >> 4;
    for (int nt = wave; nt < ntn; nt += NW) {
        f32x4 acc[MAXMT];
#pragma unroll
        for (int m = 0; m < MAXMT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *wp = W.w + (size_t)(nt * 16 + li) * Kp + 4 * g;
        const float *ap = A + (size_t)li * lda + 4 * g;
        for (int k0 = 0; k0 < Kp; k0 += 16) {
            const float4 b = *(const float4 *)(wp + k0);
#pragma unroll
            for (int m = 0; m < MAXMT; ++m)
                if (m < mt) acc[m] = mma16(*(const float4 *)(ap + (size_t)m * 16 * lda + k0), b, acc[m]);
        }
        const int col = nt * 16 + li;
        const float bias = W.b[col];
#pragma unroll
        for (int m = 0; m < MAXMT; ++m)
            if (m < mt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = m * 16 + g * 4 + r;
                    if (row < m_valid && col < n_valid) {
                        float v = act(ACT, acc[m][r] + bias) * oscale;
                        if (res) v = res[(size_t)row * ldo + col] + v;
                        out[(size_t)row * ldo + col] = v;
                    }
                }
            }
    }
}

// a chain of Linears with SiLU between them (diffusion_util.MLP): the hidden layers alternate between the two scratch regions with all
// their padded rows and columns; the caller runs the last layer.  Returns where the last hidden layer is (lda = its Np).
__device__ __forceinline__ const float *mlp_hidden(const float *A, int lda, int mt, const Lin *lin, int nhidden, float *r1, float *r2, int &lda_out) {
    const float *src = A;
    int ld = lda;
    for (int i = 0; i < nhidden; ++i) {
        float *dst = (i & 1) ? r2 : r1;
        gemm<ACT_SILU>(src, ld, mt, lin[i], dst, lin[i].Np, mt * 16, lin[i].Np, nullptr, 1.f);
        __syncthreads();
        src = dst; ld = lin[i].Np;
    }
    lda_out = ld;
    return src;
}

// LayerNorm (eps 1e-5, biased variance) of rows [0, rows) of X in place: a wave per row, lanes stride the columns
__device__ __forceinline__ void layer_norm(float *X, int ldx, int rows, int d, const float *w, const float *b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < rows; r += NW) {
        float *x = X + (size_t)r * ldx;
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += x[c];
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)d;
        float q = 0.f;
        for (int c = lane; c < d; c += 64) { const float u = x[c] - mean; q += u * u; }
        for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o, 64);
        const float rstd = 1.f / sqrtf(q / (float)d + 1e-5f);
        for (int c = lane; c < d; c += 64) x[c] = ((x[c] - mean) * rstd) * w[c] + b[c];
    }
}

// key j of the sequence takes part in the softmax (the key-padding mask of embed_conds, and the padding rows past the sequence)
__device__ __forceinline__ bool key_ok(const Net &N, int flags, int j) {
    if (j >= N.NP) return false;
    if (j >= 1 && j < 65) return (flags & F_OBS) != 0;
    if (j == 65) return (flags & F_TARGET) != 0;
    if (j >= NC && j < NC + N.nprev) return (flags & F_PREV) != 0;
    return true;
}

// self-attention of all heads: Q/K/V [NPAD][3 d] in qkv (the packed in_proj's order), the output [NPAD][d] in ao.  A wave owns one
// (head, row tile) at a time: scores through mma16 into its own LDS tile sw [16][lds], the masked softmax there, then P V through mma16.
// Every wave passes the same barriers.
__device__ __forceinline__ void attention(const Net &N, int flags, const float *qkv, float *ao, float *sb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    const int d = N.d, hd = N.hd, ld3 = 3 * d, lds = N.lds, MT = N.MT, items = N.H * MT;
    float *sw = sb + (size_t)wave * 16 * lds;
    const float scale = 1.f / sqrtf((float)hd);
    for (int it0 = 0; it0 < items; it0 += NW) {
        const int it = it0 + wave, h = it / MT, mt = it - h * MT;
        const bool live = it < items;
        if (live) {
            const float *qp = qkv + (size_t)(mt * 16 + li) * ld3 + h * hd + 4 * g;
            float4 aq[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) aq[kk] = kk * 16 < hd ? *(const float4 *)(qp + kk * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            for (int nt = 0; nt < MT; ++nt) {
                const float *kp = qkv + (size_t)(nt * 16 + li) * ld3 + d + h * hd + 4 * g;
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    if (kk * 16 < hd) acc = mma16(aq[kk], *(const float4 *)(kp + kk * 16), acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) sw[(g * 4 + r) * lds + nt * 16 + li] = acc[r] * scale;
            }
        }
        __syncthreads();
        if (live) {                                            // row li, keys g, g + 4, ..: the four groups meet through xor 16 and 32
            float *row = sw + li * lds;
            float m = -INFINITY;
            for (int j = g; j < N.NPAD; j += 4) if (key_ok(N, flags, j)) m = fmaxf(m, row[j]);
            m = fmaxf(m, __shfl_xor(m, 16, 64)); m = fmaxf(m, __shfl_xor(m, 32, 64));
            float s = 0.f;
            for (int j = g; j < N.NPAD; j += 4) {
                const float e = key_ok(N, flags, j) ? expf(row[j] - m) : 0.f;
                row[j] = e;
                s += e;
            }
            s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);
            for (int j = g; j < N.NPAD; j += 4) row[j] = row[j] / s;
        }
        __syncthreads();
        if (live) {
            for (int nt = 0; nt < (hd >> 4); ++nt) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                const float *vp = qkv + 2 * d + h * hd + nt * 16 + li;
                for (int k0 = 0; k0 < N.NPAD; k0 += 16) {
                    const float4 a = *(const float4 *)(sw + li * lds + k0 + 4 * g);
                    const float *v = vp + (size_t)(k0 + 4 * g) * ld3;
                    acc = mma16(a, make_float4(v[0], v[ld3], v[2 * ld3], v[3 * ld3]), acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) ao[(size_t)(mt * 16 + g * 4 + r) * d + h * hd + nt * 16 + li] = acc[r];
            }
        }
        __syncthreads();
    }
}

// ---- draws --------------------------------------------------------------------------------------------------------------------------
// element e of the standard-normal array of (sample idx, step): Philox4x32-10 counter (e >> 2, step << 40 | idx), Box-Muller on its two pairs
__device__ __forceinline__ float normal_at(unsigned long long seed, unsigned long long idx, unsigned step, unsigned e) {
    float u[4];
    philox4(seed, ((unsigned long long)step << 40) | idx, e >> 2, u);
    const int p = (e >> 1) & 1;
    const float r = sqrtf(-2.f * logf(1.f - u[2 * p])), a = 6.28318530717958647692f * u[2 * p + 1];
    return (e & 1) ? r * sinf(a) : r * cosf(a);
}

// the draws of (first + sample, step) as an array [n][per]: what k_mdm_cond (step 0, x_T) and k_mdm_update (step i + 1) draw in place
__global__ void k_mdm_draw(float *out, long long total, int per, unsigned long long seed, unsigned long long first, unsigned step) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long s = i / per;
    out[i] = normal_at(seed, first + (unsigned long long)s, step, (unsigned)(i - s * per));
}

// ---- k_mdm_cond ---------------------------------------------------------------------------------------------------------------------
// a valid convolution with LeakyReLU(0.01): in [Ci][Hi][Hi] -> out [Co][Ho][Ho], or (tok) the Unfold(2, 2) token layout [Ho/2 * Ho/2][Co * 4]
__device__ __forceinline__ void conv_lrelu(const float *in, int Ci, int Hi, const float *w, const float *b, int Co, int ks, float *out, bool tok) {
    const int Ho = Hi - ks + 1, n = Co * Ho * Ho;
    for (int i = threadIdx.x; i < n; i += WG) {
        const int co = i / (Ho * Ho), rem = i - co * Ho * Ho, y = rem / Ho, x = rem - y * Ho;
        float acc = 0.f;
        for (int ci = 0; ci < Ci; ++ci) {
            const float *ip = in + ((size_t)ci * Hi + y) * Hi + x, *wq = w + ((size_t)co * Ci + ci) * ks * ks;
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx) acc += ip[ky * Hi + kx] * wq[ky * ks + kx];
        }
        float v = acc + b[co];
        v = v > 0.f ? v : 0.01f * v;
        if (tok) out[(size_t)((y >> 1) * (Ho >> 1) + (x >> 1)) * (Co * 4) + co * 4 + (y & 1) * 2 + (x & 1)] = v;
        else out[i] = v;
    }
}

__global__ void __launch_bounds__(WG) k_mdm_cond(const Net *Np, Batch Bt, const float *hf, const float *target, const float *prev, const int *obs_flag,
                                                 const int *target_flag, const int *prev_flag, const int *ind, float *tokens_out,
                                                 unsigned long long *mask_out, float *x_draw, unsigned long long seed, unsigned long long first) {
    extern __shared__ float4 smem4[];
    float *sb = (float *)smem4;                                // [16][20]: the target as a row tile
    const Net &N = *Np;
    const int tid = threadIdx.x, d = N.d;
    float *r1 = Bt.scratch + (size_t)blockIdx.x * (N.r1 + N.r2), *r2 = r1 + N.r1;
    for (int s = blockIdx.x; s < Bt.n; s += gridDim.x) {
        const int fl = (obs_flag[s] ? F_OBS : 0) | (target_flag[s] ? F_TARGET : 0) | (prev_flag[s] ? F_PREV : 0) | (ind[s] ? F_IND : 0);
        if (tid == 0) Bt.flags[s] = fl;
        for (int i = tid; i < N.nprev * N.D; i += WG) Bt.prev[(size_t)s * N.nprev * N.D + i] = prev[(size_t)s * N.nprev * N.D + i];
        if (mask_out && tid < 3) {
            unsigned long long m = 0;
            for (int j = 0; j < 64; ++j) { const int k = tid * 64 + j; if (k < N.NP && !key_ok(N, fl, k)) m |= 1ull << j; }
            mask_out[(size_t)s * 3 + tid] = m;
        }
        if (x_draw) for (int e = tid; e < N.T * N.D; e += WG) x_draw[(size_t)s * N.T * N.D + e] = normal_at(seed, first + (unsigned long long)s, 0u, (unsigned)e);
        for (int i = tid; i < 16 * 20; i += WG) sb[i] = (i < N.tgt[0].K) ? target[(size_t)s * N.tgt[0].K + i] : 0.f;
        float *tk = Bt.tokens + (size_t)s * NCOND * d;
        conv_lrelu(hf + (size_t)s * PARC_MDM_GRID * PARC_MDM_GRID, 1, 31, N.conv_w[0], N.conv_b[0], 32, 5, r1, false);
        __syncthreads();
        conv_lrelu(r1, 32, 27, N.conv_w[1], N.conv_b[1], 32, 5, r2, false);
        __syncthreads();
        conv_lrelu(r2, 32, 23, N.conv_w[2], N.conv_b[2], 32, 5, r1, false);
        __syncthreads();
        conv_lrelu(r1, 32, 19, N.conv_w[3], N.conv_b[3], 64, 4, r2, true);
        __syncthreads();
        gemm<ACT_NONE>(r2, TOK_DIM, 4, N.obs, tk, d, 64, d, nullptr, (fl & F_OBS) ? 1.f : 0.f);
        __syncthreads();
        int ld;
        const float *hsrc = mlp_hidden(sb, 20, 1, N.tgt, N.ntgt, r1, r2, ld);
        gemm<ACT_NONE>(hsrc, ld, 1, N.tgt[N.ntgt], tk + (size_t)64 * d, d, 1, d, nullptr, (fl & F_TARGET) ? 1.f : 0.f);
        __syncthreads();
        if (tokens_out) for (int i = tid; i < NCOND * d; i += WG) tokens_out[(size_t)s * NCOND * d + i] = tk[i];
        __syncthreads();
    }
}

// ---- k_mdm_forward ------------------------------------------------------------------------------------------------------------------
// rows [0, n): the first pass of every sample; rows [n, 2 n) (two = 1): the second pass of guidance in the same launch, which reads x as
// the first pass leaves it (the clean previous state) and writes nothing back.
__global__ void __launch_bounds__(WG) k_mdm_forward(const Net *Np, Batch Bt, float *x, int t, int pass, int two, float *x0_out) {
    extern __shared__ float4 smem4[];
    const Net &N = *Np;
    float *X = (float *)smem4, *sb = X + (size_t)N.xrows * N.ldx;
    const int tid = threadIdx.x, d = N.d, ldx = N.ldx, T = N.T, D = N.D, MT = N.MT;
    float *r1 = Bt.scratch + (size_t)blockIdx.x * (N.r1 + N.r2), *r2 = r1 + N.r1;
    const int rows = two ? 2 * Bt.n : Bt.n;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int s = row < Bt.n ? row : row - Bt.n;
        const bool second = row >= Bt.n;
        const int cached = Bt.flags[s];
        // the pass's view of the conditions (predict_x0 :836-852)
        int flags = cached;                                    // the tokens and the mask come from the flags embed_conds saw
        bool overwrite = (cached & F_IND) != 0, writeback = true;
        if (pass == PARC_MDM_PASS_GUIDED && !second) overwrite = true;
        if (pass == PARC_MDM_PASS_UNCOND || second) {
            flags = cached & ~(F_PREV | F_IND);
            overwrite = second;                                // alone: the indicator is false; fused: x is what the first pass wrote
            writeback = false;
        }
        __syncthreads();                                       // the last sample's reads of X and sb
        // tokens: X = cat(time, heightfield, target, indicator, frames) + positional rows; the rows past the sequence are zero
        for (int i = tid; i < N.xrows * d; i += WG) {
            const int r = i / d, c = i - r * d;
            float v = 0.f;
            if (r < N.NP) {
                v = N.pe_seq[(size_t)r * d + c];
                if (r >= 1 && r < 1 + NCOND) v = Bt.tokens[((size_t)s * NCOND + r - 1) * d + c] + v;
                else if (r == 1 + NCOND) v = N.ind_embed[(size_t)((flags & F_IND) ? 1 : 0) * d + c] + v;
            }
            X[(size_t)r * ldx + c] = v;
        }
        const int ldxs = N.DP + 4;                             // the frames as row tiles: xs [TP][DP + 4], zero past T and D
        for (int i = tid; i < N.TP * N.DP; i += WG) {
            const int m = i / N.DP, k = i - m * N.DP;
            float v = 0.f;
            if (m < T && k < D) {
                float *xp = x + ((size_t)s * T + m) * D + k;
                if (m < N.nprev && overwrite) {
                    v = Bt.prev[((size_t)s * N.nprev + m) * D + k];
                    if (writeback) *xp = v;
                } else v = *xp;
            }
            sb[m * ldxs + k] = v;
        }
        // the time token: time_embed(table row t), into row 0 on top of its positional row
        gemm<ACT_SILU>(N.pe_time + (size_t)t * d, 0, 1, N.time0, r2, N.time0.Np, 16, N.time0.Np, nullptr, 1.f);
        __syncthreads();
        gemm<ACT_NONE>(r2, N.time0.Np, 1, N.time1, X, ldx, 1, d, X, 1.f);
        __syncthreads();
        int ld;
        const float *hsrc = mlp_hidden(sb, ldxs, N.TP >> 4, N.inm, N.nin, r1, r2, ld);
        gemm<ACT_NONE>(hsrc, ld, N.TP >> 4, N.inm[N.nin], X + (size_t)NC * ldx, ldx, T, d, X + (size_t)NC * ldx, 1.f);
        __syncthreads();
        for (int l = 0; l < N.L; ++l) {                        // post-norm encoder layers
            const Layer &Y = N.layer[l];
            gemm<ACT_NONE>(X, ldx, MT, Y.qkv, r1, 3 * d, N.NPAD, 3 * d, nullptr, 1.f);
            __syncthreads();
            attention(N, flags, r1, r2, sb);
            gemm<ACT_NONE>(r2, d, MT, Y.out, X, ldx, N.NPAD, d, X, 1.f);
            __syncthreads();
            layer_norm(X, ldx, N.NPAD, d, Y.n1w, Y.n1b);
            __syncthreads();
            gemm<ACT_GELU>(X, ldx, MT, Y.l1, r2, N.dh, N.NPAD, N.dh, nullptr, 1.f);
            __syncthreads();
            gemm<ACT_NONE>(r2, N.dh, MT, Y.l2, X, ldx, N.NPAD, d, X, 1.f);
            __syncthreads();
            layer_norm(X, ldx, N.NPAD, d, Y.n2w, Y.n2b);
            __syncthreads();
        }
        hsrc = mlp_hidden(X + (size_t)NC * ldx, ldx, N.TP >> 4, N.outm, N.nout, r1, r2, ld);
        gemm<ACT_NONE>(hsrc, ld, N.TP >> 4, N.outm[N.nout], x0_out + (size_t)row * T * D, D, T, D, nullptr, 1.f);
    }
}

// ---- k_mdm_update -------------------------------------------------------------------------------------------------------------------
// Joint.rot_to_dof (kin_char_model.py:83-105)
__device__ __forceinline__ void rot_to_dof(const CharTree &M, int j, Q4 q, float *dof) {
    const int t = M.jtype[j];
    if (t == PARC_JOINT_HINGE) {
        V3 ax; float ang;
        quat_to_axis_angle(q, ax, ang);
        if (M.axis[j][0] * ax.x + M.axis[j][1] * ax.y + M.axis[j][2] * ax.z < 0.f) ang = ang * -1.f;
        dof[M.dof_idx[j]] = ang;
    } else if (t == PARC_JOINT_SPHERICAL) {
        const V3 e = quat_to_exp_map(q);
        float *o = dof + M.dof_idx[j];
        o[0] = e.x; o[1] = e.y; o[2] = e.z;
    }
}

// lane per frame (mdm.py:848, :990-1008, :982-987 / :916-920).  Per lane in LDS: the frame [D], body positions [B][3], body and joint
// rotations [B][4] each.
__global__ void __launch_bounds__(UPD_T) k_mdm_update(const Net *Np, const CharTree *Mp, long long frames, const float *x0, const float *x0_nc, float gs,
                                                      float *x, int last, float c0, float ct, float cn, const float *noise, int draw,
                                                      unsigned long long seed, unsigned long long first, unsigned step, float *x0p_out) {
    extern __shared__ float4 smem4[];
    const Net &N = *Np;
    const CharTree &M = *Mp;
    const int D = N.D, T = N.T, B = M.B, J = B - 1, per = (D + 11 * B) | 1;   // an odd stride: the lanes' areas start on different LDS banks
    const long long i = (long long)blockIdx.x * UPD_T + threadIdx.x;
    if (i >= frames) return;
    float *fr = (float *)smem4 + (size_t)threadIdx.x * per, *pos = fr + D, *rot = pos + 3 * B, *jr = rot + 4 * B;
    const long long s = i / T;
    const int f = (int)(i - s * T);
    const float *mean = N.mean + (size_t)f * D, *sd = N.std + (size_t)f * D;
    for (int k = 0; k < D; ++k) {
        float v = x0[i * D + k];
        if (x0_nc) v = v + gs * (x0_nc[i * D + k] - v);
        fr[k] = v * sd[k] + mean[k];
    }
    const int o_jp = 6, o_jr = 6 + 3 * J, o_c = o_jr + M.D;
    const Q4 rq = exp_map_to_quat(ld3(fr + 3));
    for (int j = 1; j < B; ++j) st4(jr + 4 * j, dof_rot(M, j, fr + o_jr));
    fk_frame(M, ld3(fr), rq, jr, pos, rot);
    st3(fr + 3, quat_to_exp_map(rq));
    for (int k = 0; k < 3 * J; ++k) fr[o_jp + k] = pos[3 + k];
    for (int j = 1; j < B; ++j) rot_to_dof(M, j, ld4(jr + 4 * j), fr + o_jr);
    for (int k = 0; k < B; ++k) fr[o_c + k] = fminf(fmaxf(fr[o_c + k], 0.f), 1.f);
    for (int k = 0; k < D; ++k) {
        const float p = (fr[k] - mean[k]) / sd[k];
        if (x0p_out) x0p_out[i * D + k] = p;
        float v = p;
        if (!last) {
            v = c0 * p + ct * x[i * D + k];
            if (noise) v = v + cn * noise[i * D + k];
            else if (draw) v = v + cn * normal_at(seed, first + (unsigned long long)s, step, (unsigned)(f * D + k));
        }
        x[i * D + k] = v;
    }
}

struct EventList {                        // events with one lifetime, created as a run needs them (creating one does not synchronise)
    std::vector<hipEvent_t> ev;
    EventList() = default;
    EventList(const EventList &) = delete;
    EventList &operator=(const EventList &) = delete;
    ~EventList() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int ensure(size_t n) {
        while (ev.size() < n) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
        return PARC_OK;
    }
    hipEvent_t operator[](int i) const { return ev[(size_t)i]; }
    int elapsed(float &ms, int from, int to) const { HIPCHK(hipEventElapsedTime(&ms, ev[(size_t)from], ev[(size_t)to])); return PARC_OK; }
};

}  // namespace mdm

// ---- C-ABI --------------------------------------------------------------------------------------------------------------------------
// ev: cond: 0, 1; step i: 2 + 3 i .. (before forward, between, after update); grown to the longest run
struct ParcMdm : tool::CharHandle<parc::CharTree, mdm::EventList> {
    ParcMdmParams params{};
    mdm::Net net{};                       // the host's copy: dimensions, device pointers
    mdm::Net *d_net = nullptr;
    mdm::Batch batch{};
    float *d_x0 = nullptr;                // [2 max_batch][T][D]
    std::vector<float> sac, somac, pc1, pc2, pstd;
    int slots = 0, cond_slots = 0;
    size_t lds_fwd = 0, lds_upd = 0;
    bool have_conds = false, sampled = false;
    int last_steps = 0;
};

extern "C" void parc_mdm_destroy(ParcMdm *h) { tool::destroy(h); }

namespace mdm {
struct Packer {                           // the weights as the kernels read them: offsets first (as pointers), the base added after the upload
    std::vector<float> v;
    const float *raw(const float *p, size_t n) {
        const size_t at = v.size();
        v.insert(v.end(), p, p + n);
        while (v.size() & 3) v.push_back(0.f);
        return (const float *)(uintptr_t)(at * sizeof(float));
    }
    Lin lin(const float *w, const float *b, int N, int K) {
        Lin L;
        L.N = N; L.K = K; L.Np = (N + 15) & ~15; L.Kp = (K + 15) & ~15;
        const size_t at = v.size();
        v.resize(at + (size_t)L.Np * L.Kp + L.Np, 0.f);
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) v[at + (size_t)n * L.Kp + k] = w[(size_t)n * K + k];
        for (int n = 0; n < N; ++n) v[at + (size_t)L.Np * L.Kp + n] = b[n];
        L.w = (const float *)(uintptr_t)(at * sizeof(float));
        L.b = (const float *)(uintptr_t)((at + (size_t)L.Np * L.Kp) * sizeof(float));
        return L;
    }
};
static void rebase(const float *&p, const float *base) { p = (const float *)((const char *)base + (uintptr_t)p); }
static void rebase(Lin &L, const float *base) { rebase(L.w, base); rebase(L.b, base); }
}  // namespace mdm

extern "C" int parc_mdm_create(const ParcMdmParams *p, ParcMdm **out) {
    using namespace mdm;
    PARC_TRY(tool::create_args("mdm", "ParcMdmParams", p, out, 2, false));
    const ParcCharModel &cm = p->model;
    const int d = p->d_model, dh = p->d_hid, H = p->num_heads, T = p->seq_len, D = p->frame_dim;
    auto dim_ok = [](int v, int hi) { return v >= 16 && v <= hi && (v & 15) == 0; };
    if (!dim_ok(d, PARC_MDM_MAX_D_MODEL))
        return fail(PARC_ERR_INVALID, "mdm: d_model must be a multiple of 16 up to PARC_MDM_MAX_D_MODEL = " + std::to_string(PARC_MDM_MAX_D_MODEL) +
                                          " (the residual stream stays in LDS; 352 at 15 frames)");
    if (!dim_ok(dh, PARC_MDM_MAX_DIM)) return fail(PARC_ERR_INVALID, "mdm: d_hid must be a multiple of 16 up to PARC_MDM_MAX_DIM = " + std::to_string(PARC_MDM_MAX_DIM));
    if (H < 1 || d % H != 0 || (d / H != 16 && d / H != 32 && d / H != 64))
        return fail(PARC_ERR_INVALID, "mdm: head_dim = d_model / num_heads must be 16, 32 or 64");
    if (p->num_layers < 1 || p->num_layers > PARC_MDM_MAX_LAYERS) return fail(PARC_ERR_INVALID, "mdm: num_layers must be 1 .. PARC_MDM_MAX_LAYERS = " + std::to_string(PARC_MDM_MAX_LAYERS));
    if (T < 1 || T > PARC_MDM_MAX_SEQ) return fail(PARC_ERR_INVALID, "mdm: seq_len must be 1 .. PARC_MDM_MAX_SEQ = " + std::to_string(PARC_MDM_MAX_SEQ));
    if (p->num_prev_states < 0 || p->num_prev_states >= T) return fail(PARC_ERR_INVALID, "mdm: num_prev_states must be < seq_len");
    if (p->diffusion_timesteps < 1) return fail(PARC_ERR_INVALID, "mdm: diffusion_timesteps must be >= 1");
    if (p->target_dim != 2) return fail(PARC_ERR_INVALID, "mdm: target_dim must be 2 (target_type XY_DIR)");
    if (D != 6 + 3 * (cm.num_bodies - 1) + cm.dof_size + cm.num_bodies)
        return fail(PARC_ERR_INVALID, "mdm: frame_dim must be ROOT_POS, ROOT_ROT, JOINT_POS, JOINT_ROT, CONTACTS of the character: " +
                                          std::to_string(6 + 3 * (cm.num_bodies - 1) + cm.dof_size + cm.num_bodies));
    if (p->max_batch < 1) return fail(PARC_ERR_INVALID, "mdm: max_batch must be >= 1");
    const int32_t *lists[3] = {p->target_hidden, p->in_hidden, p->out_hidden};
    const int counts[3] = {p->num_target_hidden, p->num_in_hidden, p->num_out_hidden};
    int maxw = 16;
    for (int m = 0; m < 3; ++m) {
        if (counts[m] < 0 || counts[m] > PARC_MDM_MAX_HIDDEN) return fail(PARC_ERR_INVALID, "mdm: an MLP has more than PARC_MDM_MAX_HIDDEN hidden layers");
        for (int i = 0; i < counts[m]; ++i) {
            if (lists[m][i] < 1 || lists[m][i] > PARC_MDM_MAX_WIDTH) return fail(PARC_ERR_INVALID, "mdm: an MLP hidden width must be 1 .. PARC_MDM_MAX_WIDTH = " + std::to_string(PARC_MDM_MAX_WIDTH));
            maxw = std::max(maxw, (lists[m][i] + 15) & ~15);
        }
    }
    if (!p->weights_host || !p->weight_offsets_host || !p->mean_host || !p->std_host || !p->sqrt_alphas_cumprod_host || !p->sqrt_one_minus_alphas_cumprod_host ||
        !p->posterior_mean_coef1_host || !p->posterior_mean_coef2_host || !p->posterior_std_host)
        return fail(PARC_ERR_INVALID, "mdm: null array");
    for (long long i = 0; i < (long long)T * D; ++i)
        if (!std::isfinite(p->mean_host[i]) || !std::isfinite(p->std_host[i]) || p->std_host[i] == 0.f) return fail(PARC_ERR_INVALID, "mdm: the feature mean / std must be finite, the std non-zero");
    parc::CharTree M;
    PARC_TRY(tool::char_tree("mdm", cm, M));

    Net N{};
    N.d = d; N.H = H; N.hd = d / H; N.dh = dh; N.L = p->num_layers; N.T = T; N.nprev = p->num_prev_states; N.D = D;
    N.DP = (D + 15) & ~15; N.TP = (T + 15) & ~15; N.NP = NC + T; N.NPAD = (N.NP + 15) & ~15; N.MT = N.NPAD >> 4;
    N.xrows = std::max(N.NPAD, NC + N.TP); N.ldx = d + 4; N.lds = N.NPAD + 4; N.timesteps = p->diffusion_timesteps;
    N.r1 = std::max<long long>({(long long)N.NPAD * 3 * d, (long long)N.TP * maxw, (long long)CONV_A, 16LL * maxw});
    N.r2 = std::max<long long>({(long long)N.NPAD * std::max(d, dh), (long long)N.TP * maxw, (long long)CONV_B, 16LL * maxw, 16LL * d});
    const size_t sb_floats = std::max<size_t>({(size_t)NW * 16 * N.lds, (size_t)N.TP * (N.DP + 4), (size_t)16 * 20});
    const size_t lds_fwd = ((size_t)N.xrows * N.ldx + sb_floats) * sizeof(float);
    if (lds_fwd > 160 * 1024)
        return fail(PARC_ERR_INVALID, "mdm: the residual stream of " + std::to_string(N.NP) + " tokens of d_model " + std::to_string(d) + " with the attention tiles needs " +
                                          std::to_string(lds_fwd) + " B of LDS; a workgroup has 163840");

    // the tensors, in the header's order, each checked against the size its dimensions give
    const int n_expected = 8 + 2 + 1 + 2 + 4 + 12 * N.L + 2 * (counts[0] + 1) + 2 * (counts[1] + 1) + 2 * (counts[2] + 1);
    if (p->num_tensors != n_expected) return fail(PARC_ERR_INVALID, "mdm: " + std::to_string(p->num_tensors) + " weight tensors given, this shape has " + std::to_string(n_expected));
    int cur = 0;
    bool bad = false;
    std::string bad_at;
    auto take = [&](long long n, const char *name) -> const float * {
        const long long a = p->weight_offsets_host[cur], b = p->weight_offsets_host[cur + 1];
        if (b - a != n && !bad) { bad = true; bad_at = std::string(name) + " (tensor " + std::to_string(cur) + "): " + std::to_string(b - a) + " values, expected " + std::to_string(n); }
        ++cur;
        return p->weights_host + a;
    };
    Packer P;
    const int cdim[4][3] = {{32, 1, 5}, {32, 32, 5}, {32, 32, 5}, {64, 32, 4}};
    const float *cw[4], *cb[4];
    for (int c = 0; c < 4; ++c) { cw[c] = take((long long)cdim[c][0] * cdim[c][1] * cdim[c][2] * cdim[c][2], "conv weight"); cb[c] = take(cdim[c][0], "conv bias"); }
    const float *ow = take((long long)d * TOK_DIM, "_obs_embed.weight"), *ob = take(d, "_obs_embed.bias");
    const float *ie = take(2LL * d, "indicator embedding"), *pt = take((long long)p->diffusion_timesteps * d, "timestep table"), *ps = take((long long)N.NP * d, "positional table");
    const float *t0w = take((long long)d * d, "time_embed.0.weight"), *t0b = take(d, "time_embed.0.bias");
    const float *t1w = take((long long)d * d, "time_embed.2.weight"), *t1b = take(d, "time_embed.2.bias");
    struct LW { const float *p[12]; } lw[PARC_MDM_MAX_LAYERS];
    for (int l = 0; l < N.L; ++l) {
        const long long sz[12] = {3LL * d * d, 3LL * d, (long long)d * d, d, (long long)dh * d, dh, (long long)d * dh, d, d, d, d, d};
        for (int k = 0; k < 12; ++k) lw[l].p[k] = take(sz[k], "encoder layer tensor");
    }
    struct MW { const float *w[PARC_MDM_MAX_HIDDEN + 1], *b[PARC_MDM_MAX_HIDDEN + 1]; int dims[PARC_MDM_MAX_HIDDEN + 2]; } mw[3];
    const int first_dim[3] = {p->target_dim, D, d}, last_dim[3] = {d, d, D};
    for (int m = 0; m < 3; ++m) {
        mw[m].dims[0] = first_dim[m];
        for (int i = 0; i < counts[m]; ++i) mw[m].dims[i + 1] = lists[m][i];
        mw[m].dims[counts[m] + 1] = last_dim[m];
        for (int i = 0; i <= counts[m]; ++i) { mw[m].w[i] = take((long long)mw[m].dims[i + 1] * mw[m].dims[i], "MLP weight"); mw[m].b[i] = take(mw[m].dims[i + 1], "MLP bias"); }
    }
    if (bad) return fail(PARC_ERR_INVALID, "mdm: " + bad_at);
    for (long long i = p->weight_offsets_host[0]; i < p->weight_offsets_host[p->num_tensors]; ++i)
        if (!std::isfinite(p->weights_host[i])) return fail(PARC_ERR_INVALID, "mdm: a weight is not finite");

    for (int c = 0; c < 4; ++c) { N.conv_w[c] = P.raw(cw[c], (size_t)cdim[c][0] * cdim[c][1] * cdim[c][2] * cdim[c][2]); N.conv_b[c] = P.raw(cb[c], cdim[c][0]); }
    N.obs = P.lin(ow, ob, d, TOK_DIM);
    N.ind_embed = P.raw(ie, 2 * (size_t)d); N.pe_time = P.raw(pt, (size_t)p->diffusion_timesteps * d); N.pe_seq = P.raw(ps, (size_t)N.NP * d);
    N.time0 = P.lin(t0w, t0b, d, d); N.time1 = P.lin(t1w, t1b, d, d);
    for (int l = 0; l < N.L; ++l) {
        Layer &Y = N.layer[l];
        Y.qkv = P.lin(lw[l].p[0], lw[l].p[1], 3 * d, d); Y.out = P.lin(lw[l].p[2], lw[l].p[3], d, d);
        Y.l1 = P.lin(lw[l].p[4], lw[l].p[5], dh, d); Y.l2 = P.lin(lw[l].p[6], lw[l].p[7], d, dh);
        Y.n1w = P.raw(lw[l].p[8], d); Y.n1b = P.raw(lw[l].p[9], d); Y.n2w = P.raw(lw[l].p[10], d); Y.n2b = P.raw(lw[l].p[11], d);
    }
    N.ntgt = counts[0]; N.nin = counts[1]; N.nout = counts[2];
    Lin *mlps[3] = {N.tgt, N.inm, N.outm};
    for (int m = 0; m < 3; ++m)
        for (int i = 0; i <= counts[m]; ++i) mlps[m][i] = P.lin(mw[m].w[i], mw[m].b[i], mw[m].dims[i + 1], mw[m].dims[i]);
    N.mean = P.raw(p->mean_host, (size_t)T * D); N.std = P.raw(p->std_host, (size_t)T * D);

    return tool::create("mdm", p->device, out, [&](ParcMdm &h) -> int {
        h.params = *p; h.host_model = M;
        h.params.weights_host = nullptr; h.params.weight_offsets_host = nullptr;   // the caller's buffers are not kept
        const int TS = p->diffusion_timesteps;
        h.sac.assign(p->sqrt_alphas_cumprod_host, p->sqrt_alphas_cumprod_host + TS);
        h.somac.assign(p->sqrt_one_minus_alphas_cumprod_host, p->sqrt_one_minus_alphas_cumprod_host + TS);
        h.pc1.assign(p->posterior_mean_coef1_host, p->posterior_mean_coef1_host + TS);
        h.pc2.assign(p->posterior_mean_coef2_host, p->posterior_mean_coef2_host + TS);
        h.pstd.assign(p->posterior_std_host, p->posterior_std_host + TS);
        float *d_w = nullptr;
        PARC_TRY(h.mem.alloc(d_w, (long long)P.v.size(), P.v.data()));
        for (int c = 0; c < 4; ++c) { rebase(N.conv_w[c], d_w); rebase(N.conv_b[c], d_w); }
        rebase(N.obs, d_w); rebase(N.time0, d_w); rebase(N.time1, d_w);
        rebase(N.ind_embed, d_w); rebase(N.pe_time, d_w); rebase(N.pe_seq, d_w); rebase(N.mean, d_w); rebase(N.std, d_w);
        for (int l = 0; l < N.L; ++l) {
            Layer &Y = N.layer[l];
            rebase(Y.qkv, d_w); rebase(Y.out, d_w); rebase(Y.l1, d_w); rebase(Y.l2, d_w);
            rebase(Y.n1w, d_w); rebase(Y.n1b, d_w); rebase(Y.n2w, d_w); rebase(Y.n2b, d_w);
        }
        for (int m = 0; m < 3; ++m)
            for (int i = 0; i <= counts[m]; ++i) rebase(mlps[m][i], d_w);
        h.net = N;
        PARC_TRY(h.mem.alloc(h.d_net, 1, &N));
        PARC_TRY(model_upload(h.mem, M, h.d_model));
        // the grid of k_mdm_forward: the workgroups one launch keeps resident (the scratch is indexed by the workgroup)
        h.lds_fwd = lds_fwd;
        h.lds_upd = (size_t)UPD_T * ((D + 11 * M.B) | 1) * sizeof(float);
        HIPCHK(hipFuncSetAttribute((const void *)k_mdm_forward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h.lds_fwd));
        HIPCHK(hipFuncSetAttribute((const void *)k_mdm_update, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h.lds_upd));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, p->device));
        int per_cu = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_mdm_forward, WG, h.lds_fwd));
        if (per_cu < 1) return fail(PARC_ERR_INVALID, "mdm: k_mdm_forward does not fit a compute unit with " + std::to_string(h.lds_fwd) + " B of LDS");
        h.slots = std::min(2 * p->max_batch, per_cu * prop.multiProcessorCount);
        const long long B = p->max_batch;
        PARC_TRY(h.mem.alloc(h.batch.tokens, B * NCOND * d));
        PARC_TRY(h.mem.alloc(h.batch.prev, B * std::max(1, N.nprev) * D));
        PARC_TRY(h.mem.alloc_fill(h.batch.flags, B));
        PARC_TRY(h.mem.alloc_fill(h.batch.scratch, (long long)h.slots * (N.r1 + N.r2)));
        PARC_TRY(h.mem.alloc_fill(h.d_x0, 2 * B * T * D));
        return h.ev.ensure(2 + 3 * 4);
    });
}

static int mdm_check_conds(ParcMdm *h, const ParcMdmConds *c) {
    if (!h || !c) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (c->n < 1 || c->n > h->params.max_batch) return fail(PARC_ERR_INVALID, "mdm: the batch must be 1 .. max_batch = " + std::to_string(h->params.max_batch));
    // with num_prev_states = 0 the previous state is [n][0][D]: nothing reads it, and an empty tensor's pointer is null
    if (!c->hf || !c->target || (!c->prev_state && h->params.num_prev_states > 0) || !c->obs_flag || !c->target_flag || !c->prev_state_flag || !c->noise_ind)
        return fail(PARC_ERR_INVALID, "mdm: null condition array");
    return PARC_OK;
}

static int mdm_launch_cond(ParcMdm *h, const ParcMdmConds *c, float *tokens_out, uint64_t *mask_out, float *x_draw, uint64_t seed, uint64_t first, hipStream_t st) {
    h->batch.n = c->n;
    const int grid = std::min(c->n, h->slots);
    PARC_TRY(tool::launch(mdm::k_mdm_cond, dim3((unsigned)grid), dim3(mdm::WG), 16 * 20 * sizeof(float), st, h->d_net, h->batch, c->hf, c->target, c->prev_state,
                       c->obs_flag, c->target_flag, c->prev_state_flag, c->noise_ind, tokens_out, (unsigned long long *)mask_out, x_draw,
                       (unsigned long long)seed, (unsigned long long)first));
    h->have_conds = true;
    return PARC_OK;
}

extern "C" int parc_mdm_embed_conds(ParcMdm *h, const ParcMdmConds *c, float *tokens_out, uint64_t *mask_out, void *stream) {
    PARC_TRY(mdm_check_conds(h, c));
    HIPCHK(hipSetDevice(h->device));
    return mdm_launch_cond(h, c, tokens_out, mask_out, nullptr, 0, 0, (hipStream_t)stream);
}

static int mdm_launch_forward(ParcMdm *h, float *x, int t, int pass, int two, float *x0_out, hipStream_t st) {
    const int rows = two ? 2 * h->batch.n : h->batch.n;
    PARC_TRY(tool::launch(mdm::k_mdm_forward, dim3((unsigned)std::min(rows, h->slots)), dim3(mdm::WG), h->lds_fwd, st, h->d_net, h->batch, x, t, pass, two, x0_out));
    return PARC_OK;
}

extern "C" int parc_mdm_forward(ParcMdm *h, float *x, int32_t t, int32_t pass, float *x0_out, void *stream) {
    if (!h || !x || !x0_out) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (!h->have_conds) return fail(PARC_ERR_STATE, "mdm: parc_mdm_embed_conds first");
    if (t < 0 || t >= h->params.diffusion_timesteps) return fail(PARC_ERR_INVALID, "mdm: t must be 0 .. diffusion_timesteps - 1");
    if (pass < PARC_MDM_PASS_PLAIN || pass > PARC_MDM_PASS_UNCOND) return fail(PARC_ERR_INVALID, "mdm: pass must be PARC_MDM_PASS_PLAIN, _GUIDED or _UNCOND");
    HIPCHK(hipSetDevice(h->device));
    return mdm_launch_forward(h, x, t, pass, 0, x0_out, (hipStream_t)stream);
}

static int mdm_launch_update(ParcMdm *h, int n, const float *x0, const float *x0_nc, float gs, float *x, int last, float c0, float ct, float cn, const float *noise,
                             int draw, uint64_t seed, uint64_t first, unsigned step, float *x0p, hipStream_t st) {
    const long long frames = (long long)n * h->net.T;
    PARC_TRY(tool::launch(mdm::k_mdm_update, dim3(blocks(frames, mdm::UPD_T)), dim3(mdm::UPD_T), h->lds_upd, st, h->d_net, h->d_model, frames, x0, x0_nc, gs, x, last, c0,
                       ct, cn, noise, draw, (unsigned long long)seed, (unsigned long long)first, step, x0p));
    return PARC_OK;
}

extern "C" int parc_mdm_update(ParcMdm *h, int32_t n, const float *x0, const float *x0_uncond, float guidance_scale, float *x, int32_t last, float c0, float ct,
                               float cn, const float *noise, float *x0_proj_out, void *stream) {
    if (!h || !x0 || !x) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (n < 1) return fail(PARC_ERR_INVALID, "mdm: n must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    return mdm_launch_update(h, n, x0, x0_uncond, guidance_scale, x, last != 0, c0, ct, cn, noise, 0, 0, 0, 0u, x0_proj_out, (hipStream_t)stream);
}

extern "C" int parc_mdm_sample(ParcMdm *h, const ParcMdmConds *c, const ParcMdmSampleArgs *a, void *stream) {
    PARC_TRY(mdm_check_conds(h, c));
    if (!a || !a->x) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (a->mode != PARC_MDM_DDIM && a->mode != PARC_MDM_DDPM) return fail(PARC_ERR_INVALID, "mdm: mode must be PARC_MDM_DDIM or PARC_MDM_DDPM");
    if (a->num_steps < 1 || a->num_steps > PARC_MDM_MAX_STEPS || !a->timesteps_host)
        return fail(PARC_ERR_INVALID, "mdm: num_steps must be 1 .. PARC_MDM_MAX_STEPS = " + std::to_string(PARC_MDM_MAX_STEPS));
    const int TS = h->params.diffusion_timesteps;
    for (int i = 0; i < a->num_steps; ++i) {
        const int t = a->timesteps_host[i];
        if (t < 0 || t >= TS) return fail(PARC_ERR_INVALID, "mdm: a timestep lies outside 0 .. diffusion_timesteps - 1");
        if (a->mode == PARC_MDM_DDIM && t != 0 && (a->stride < 1 || t - a->stride < 0))
            return fail(PARC_ERR_INVALID, "mdm: DDIM step t = " + std::to_string(t) + " with stride " + std::to_string(a->stride) + " has no next timestep");
    }
    if (a->mode == PARC_MDM_DDPM && !a->noise && !a->draw) return fail(PARC_ERR_INVALID, "mdm: DDPM needs injected noise or draw");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int n = c->n;
    const long long per = (long long)n * h->net.T * h->net.D;
    PARC_TRY(h->ev.ensure(2 + 3 * (size_t)a->num_steps));
    HIPCHK(hipEventRecord(h->ev[0], st));
    PARC_TRY(mdm_launch_cond(h, c, nullptr, nullptr, a->draw ? a->x : nullptr, a->seed, a->first_index, st));
    HIPCHK(hipEventRecord(h->ev[1], st));
    for (int i = 0; i < a->num_steps; ++i) {
        const int t = a->timesteps_host[i];
        HIPCHK(hipEventRecord(h->ev[2 + 3 * i], st));
        PARC_TRY(mdm_launch_forward(h, a->x, t, a->use_guidance ? PARC_MDM_PASS_GUIDED : PARC_MDM_PASS_PLAIN, a->use_guidance != 0, h->d_x0, st));
        HIPCHK(hipEventRecord(h->ev[3 + 3 * i], st));
        float c0 = 0.f, ct = 0.f, cn = 0.f;
        const bool last = t == 0;                              // the reference returns before it reads the tables (next_t = -stride there)
        if (!last && a->mode == PARC_MDM_DDIM) {               // mdm.py:982-985, fp32 in that order
            const int nt = t - a->stride;
            const float numer = h->sac[t] * h->somac[nt], denom = h->somac[t];
            c0 = h->sac[nt] - numer / denom;
            ct = h->somac[nt] / h->somac[t];
        } else if (!last) { c0 = h->pc1[t]; ct = h->pc2[t]; cn = h->pstd[t]; }
        const bool ddpm = a->mode == PARC_MDM_DDPM && !last;
        PARC_TRY(mdm_launch_update(h, n, h->d_x0, a->use_guidance ? h->d_x0 + per : nullptr, a->guidance_scale, a->x, last, c0, ct, cn,
                                   ddpm && a->noise ? a->noise + (long long)i * per : nullptr, ddpm && !a->noise, a->seed, a->first_index, (unsigned)(i + 1), nullptr, st));
        HIPCHK(hipEventRecord(h->ev[4 + 3 * i], st));
        if (a->keep) HIPCHK(hipMemcpyAsync(a->keep + (long long)i * per, a->x, (size_t)per * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    h->sampled = true; h->last_steps = a->num_steps;
    return PARC_OK;
}

extern "C" int parc_mdm_draw_noise(ParcMdm *h, int32_t n, uint64_t seed, uint64_t first_index, uint32_t step, float *out, void *stream) {
    if (!h || !out) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (n < 1) return fail(PARC_ERR_INVALID, "mdm: n must be >= 1");
    HIPCHK(hipSetDevice(h->device));
    const int per = h->net.T * h->net.D;
    const long long total = (long long)n * per;
    PARC_TRY(tool::launch(mdm::k_mdm_draw, dim3(blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, out, total, per, (unsigned long long)seed,
                       (unsigned long long)first_index, (unsigned)step));
    return PARC_OK;
}

extern "C" int parc_mdm_kernel_times(ParcMdm *h, float *ms3) {
    if (!h || !ms3) return fail(PARC_ERR_INVALID, "mdm: null argument");
    if (!h->sampled) return fail(PARC_ERR_STATE, "mdm: nothing sampled yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev[4 + 3 * (h->last_steps - 1)]));
    PARC_TRY(h->ev.elapsed(ms3[0], 0, 1));
    ms3[1] = ms3[2] = 0.f;
    for (int i = 0; i < h->last_steps; ++i) {
        float a = 0.f, b = 0.f;
        PARC_TRY(h->ev.elapsed(a, 2 + 3 * i, 3 + 3 * i));
        PARC_TRY(h->ev.elapsed(b, 3 + 3 * i, 4 + 3 * i));
        ms3[1] += a; ms3[2] += b;
    }
    return PARC_OK;
}

extern "C" int parc_mdm_describe(ParcMdm *h, int64_t *out3) {
    if (!h || !out3) return fail(PARC_ERR_INVALID, "mdm: null argument");
    out3[0] = (int64_t)h->lds_fwd; out3[1] = h->slots; out3[2] = h->net.r1 + h->net.r2;
    return PARC_OK;
}
