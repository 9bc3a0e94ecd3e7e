// In-loop wav2vec2 audio encoder (wav2vec2.py): the kernels of the convolutional front end that the grouped GEMM does not cover.
// Reference: src/feature_extractors/audio_wav2vec2/embeddings.py:52-91 runs torchaudio's WAV2VEC2_BASE and mean-pools the valid frames.
//
//   conv layer 0 + GroupNorm(C, C) + GELU   three launches: per-(utterance, channel, frame chunk) statistics of the 10-tap conv, a
//                                           fixed-order Chan merge per (utterance, channel), and a pass that recomputes the conv,
//                                           normalises, applies the affine and GELU and writes the activation (the pre-norm tensor
//                                           is never stored).  The statistics cover frames 0 .. T0-1 of the PADDED batch, as
//                                           torch.nn.GroupNorm over the zero-padded waveform does.
//   feature LayerNorm                       reads the pitched rows b * P + t of the conv stack, writes the compact rows b * S + t
//   positional convolution                  implicit GEMM per (utterance, group, 64-frame tile) on MFMA, weights streamed over taps
//   masked mean pool                        [B, S, d] -> [B, d] over the first len_b frames
//
// Activations are channels-last ([frame][channel]).  Everything is deterministic: no atomics, fixed reduction orders.
#include <type_traits>

#include "common.h"
#include "ops.h"

namespace {

constexpr int NTHR = 256;
constexpr int CONV0_FCH = 128;                                   // frames per statistics / apply chunk
constexpr int CONV0_LDS = (CONV0_FCH - 1) * M2F_W2V_CONV0_MAX_STRIDE + M2F_W2V_CONV0_MAX_TAPS;

// waveform samples of one frame chunk in LDS; samples at or past N read as zero (the reference's zero padding)
__device__ __forceinline__ void conv0_stage(float* xs, const float* __restrict__ wave, int N, int b, int f0, int s0) {
    const float* w = wave + (size_t)b * N;
    const int base = f0 * s0;
    for (int i = threadIdx.x; i < CONV0_LDS; i += NTHR) xs[i] = base + i < N ? w[base + i] : 0.f;
    __syncthreads();
}

// NT taps held in registers (NT = k0 for the wav2vec2 kernel of 10 taps, else the maximum with zero taps behind k0)
template <int NT>
__device__ __forceinline__ void conv0_taps(float (&wk)[NT], const float* __restrict__ w0, int c, int k0) {
#pragma unroll
    for (int j = 0; j < NT; ++j) wk[j] = j < k0 ? w0[c * k0 + j] : 0.f;
}

template <int NT>
__device__ __forceinline__ float conv0_at(const float* xs, const float (&wk)[NT], int f, int s0) {
    const float* x = xs + f * s0;
    float y = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) y = fmaf(wk[j], x[j], y);
    return y;
}

// partial[(b * nchunk + ch) * C + c] = (mean, M2) of frames ch * FCH .. min(T0, ch * FCH + FCH) - 1; two passes over the chunk
template <int NT>
__global__ __launch_bounds__(NTHR) void m2f_w2v_conv0_stats_kernel(const float* __restrict__ wave, const float* __restrict__ w0, int N,
                                                                   int k0, int s0, int C, int T0, float2* __restrict__ partial) {
    __shared__ float xs[CONV0_LDS];
    const int ch = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
    const int f0 = ch * CONV0_FCH, nf = min(CONV0_FCH, T0 - f0);
    conv0_stage(xs, wave, N, b, f0, s0);
    for (int c = threadIdx.x; c < C; c += NTHR) {
        float wk[NT];
        conv0_taps(wk, w0, c, k0);
        float s = 0.f;
        for (int f = 0; f < nf; ++f) s += conv0_at(xs, wk, f, s0);
        const float mean = s / (float)nf;
        float m2 = 0.f;
        for (int f = 0; f < nf; ++f) {
            const float d = conv0_at(xs, wk, f, s0) - mean;
            m2 = fmaf(d, d, m2);
        }
        partial[((size_t)b * nchunk + ch) * C + c] = make_float2(mean, m2);
    }
}

// stats[b * C + c] = (mean, rstd) over T0 frames: chunk partials merged in chunk order (Chan et al.)
__global__ __launch_bounds__(NTHR) void m2f_w2v_conv0_merge_kernel(const float2* __restrict__ partial, int nchunk, int C, int T0, float eps,
                                                                   float2* __restrict__ stats) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * NTHR + threadIdx.x;
    if (c >= C) return;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
        const float2 p = partial[((size_t)b * nchunk + ch) * C + c];
        const float nb = (float)min(CONV0_FCH, T0 - ch * CONV0_FCH), nn = n + nb;
        const float d = p.x - mean;
        mean = fmaf(d, nb / nn, mean);
        m2 = m2 + p.y + d * d * (n * nb / nn);
        n = nn;
    }
    stats[(size_t)b * C + c] = make_float2(mean, rsqrtf(m2 / n + eps));
}

// out row b * P0 + t = GELU(GroupNorm(conv0)) for t < T0, zeros for T0 <= t < P0 (the pitch's slack rows); fp32 or bf16 output
template <int NT, bool OUT16>
__global__ __launch_bounds__(NTHR) void m2f_w2v_conv0_apply_kernel(const float* __restrict__ wave, const float* __restrict__ w0, int N,
                                                                   int k0, int s0, int C, int T0, int P0, const float2* __restrict__ stats,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ out32, uint16_t* __restrict__ out16) {
    __shared__ float xs[CONV0_LDS];
    const int ch = blockIdx.x, b = blockIdx.y;
    const int f0 = ch * CONV0_FCH, nf = min(CONV0_FCH, P0 - f0), nv = max(0, min(nf, T0 - f0));
    conv0_stage(xs, wave, N, b, f0, s0);
    const size_t row0 = (size_t)b * P0 + f0;
    for (int c = threadIdx.x; c < C; c += NTHR) {
        float wk[NT];
        conv0_taps(wk, w0, c, k0);
        const float2 st = stats[(size_t)b * C + c];
        const float sc = st.y * gamma[c], sh = fmaf(-st.x, sc, beta[c]);
        for (int f = 0; f < nf; ++f) {
            const float y = f < nv ? m2f_gelu<false>(fmaf(conv0_at(xs, wk, f, s0), sc, sh)) : 0.f;
            if constexpr (OUT16) out16[(row0 + f) * C + c] = m2f_bf16_bits(y);
            else out32[(row0 + f) * C + c] = y;
        }
    }
}

// LayerNorm over C channels of row b * P + t of x, written to row b * S + t of out32 (and of out16 when given); one wave per row
__global__ __launch_bounds__(NTHR) void m2f_w2v_feat_ln_kernel(const float* __restrict__ x, int B, int S, int P, int C,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               float* __restrict__ out32, uint16_t* __restrict__ out16) {
    constexpr int PER = M2F_W2V_FEAT_MAX_C / 64;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6);
    if (r >= B * S) return;
    const int b = r / S, t = r - b * S;
    const float* src = x + ((size_t)b * P + t) * C;
    float v[PER];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? src[c] : 0.f;
        s += v[i];
    }
    const float mean = m2f_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + 64 * i;
        const float d = c < C ? v[i] - mean : 0.f;
        q = fmaf(d, d, q);
    }
    const float rstd = rsqrtf(m2f_wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            const float y = fmaf((v[i] - mean) * rstd, gamma[c], beta[c]);
            out32[(size_t)r * C + c] = y;
            if (out16) out16[(size_t)r * C + c] = m2f_bf16_bits(y);
        }
    }
}

// ---- positional convolution ----------------------------------------------------------------------------------------------------
// out[b*S + t, g*CG + o] = GELU(bias + sum_{k < K, c < CG} x[t + k - K/2, g*CG + c] * W[g*CG + o, c, k]) + x[t, g*CG + o]
// with x rows at or past len_b (and outside 0 .. S-1) read as zero, the residual included (the reference zeroes padded frames first).
// One workgroup = 4 waves = 64 frames of one (utterance, group); wave w owns frames 16 w .. 16 w + 15 and all CG = 16 NJ outputs.
// The input window (64 + K - 1 rows x CG channels) sits in LDS as fp32; the weights, packed as [G][K][CG (o)][CG (c)], are streamed
// through LDS PC_TAPS taps at a time.  fp32 mode: v_mfma_f32_16x16x4_f32; bf16 mode: operands rounded to bf16 (weights arrive as
// bf16), v_mfma_f32_16x16x16_bf16, fp32 accumulation.
constexpr int PC_TILE = 64;
constexpr int PC_TAPS = 4;
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int NJ, bool BF16>
__global__ __launch_bounds__(NTHR) void m2f_w2v_pos_conv_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                                const void* __restrict__ wpk, const float* __restrict__ bias,
                                                                float* __restrict__ out, int S, int d, int K) {
    constexpr int CG = 16 * NJ, XS = CG + 4;                    // (row pitch padded by 4 floats against LDS bank conflicts)
    typedef typename std::conditional<BF16, uint16_t, float>::type WT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xw = smem;                                           // [PC_TILE + K - 1][XS]
    WT* ws = reinterpret_cast<WT*>(smem + (size_t)(PC_TILE + K - 1) * XS);   // [PC_TAPS][CG][XS]
    const int t0 = blockIdx.x * PC_TILE, g = blockIdx.y, b = blockIdx.z;
    const int pad = K / 2;
    const int len = min(max(lengths[b], 0), S);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15, lq = lane >> 4;
    const float* xb = x + (size_t)b * S * d + (size_t)g * CG;
    const int rows = PC_TILE + K - 1;
    for (int i = tid; i < rows * CG; i += NTHR) {
        const int r = i / CG, c = i - r * CG, tf = t0 - pad + r;
        xw[r * XS + c] = tf >= 0 && tf < len ? xb[(size_t)tf * d + c] : 0.f;
    }
    const WT* wg = reinterpret_cast<const WT*>(wpk) + (size_t)g * K * CG * CG;
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += PC_TAPS) {
        __syncthreads();                                        // (previous taps consumed; first trip: the window is written)
        const int nt = min(PC_TAPS, K - k0);
        for (int i = tid; i < PC_TAPS * CG * CG; i += NTHR) {
            const int kk = i / (CG * CG), rem = i - kk * CG * CG, o = rem / CG, c = rem - o * CG;
            ws[(kk * CG + o) * XS + c] = kk < nt ? wg[(size_t)(k0 + kk) * CG * CG + rem] : WT(0);
        }
        __syncthreads();
        for (int kk = 0; kk < nt; ++kk) {
            const float* xr = xw + (wv * 16 + l16 + k0 + kk) * XS;
            const WT* wr = ws + (size_t)kk * CG * XS;
            if constexpr (BF16) {
#pragma unroll
                for (int cc = 0; cc < CG; cc += 16) {
                    const f32x4 xa = *reinterpret_cast<const f32x4*>(xr + cc + 4 * lq);
                    const s16x4 a = {(short)m2f_bf16_bits(xa[0]), (short)m2f_bf16_bits(xa[1]), (short)m2f_bf16_bits(xa[2]),
                                     (short)m2f_bf16_bits(xa[3])};
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const s16x4 bv = *reinterpret_cast<const s16x4*>(wr + (j * 16 + l16) * XS + cc + 4 * lq);
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, bv, acc[j], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int cc = 0; cc < CG; cc += 4) {
                    const float a = xr[cc + lq];
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[(j * 16 + l16) * XS + cc + lq], acc[j], 0, 0, 0);
                }
            }
        }
    }
    // accumulator element r of lane: frame 16 wv + 4 lq + r, output channel 16 j + l16
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = g * CG + j * 16 + l16;
        const float bj = bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int fl = wv * 16 + 4 * lq + r, t = t0 + fl;
            if (t < S) {
                const float res = t < len ? xw[(fl + pad) * XS + j * 16 + l16] : 0.f;
                out[((size_t)b * S + t) * d + col] = m2f_gelu<false>(acc[j][r] + bj) + res;
            }
        }
    }
}

// out[b, c] = mean of x[b*S + t, c] over t < len_b (fixed order; len_b <= 0 gives zeros)
__global__ __launch_bounds__(NTHR) void m2f_w2v_masked_mean_kernel(const float* __restrict__ x, const int* __restrict__ lengths, int S, int d,
                                                                   float* __restrict__ out) {
    const int b = blockIdx.y, c = blockIdx.x * NTHR + threadIdx.x;
    if (c >= d) return;
    const int len = min(lengths[b], S);
    const float* xb = x + (size_t)b * S * d + c;
    float s = 0.f;
    for (int t = 0; t < len; ++t) s += xb[(size_t)t * d];
    out[(size_t)b * d + c] = len > 0 ? s / (float)len : 0.f;
}

template <int NT>
static void conv0_launch(const float* wave, int B, int N, const float* w0, int k0, int s0, int C, int T0, int P0, const float* gamma,
                         const float* beta, float eps, float2* part, float2* st, float* out32, uint16_t* out16, dim3 grid, int nch,
                         hipStream_t stream) {
    auto stats = m2f_w2v_conv0_stats_kernel<NT>;
    hipLaunchKernelGGL(stats, dim3(nch, B), dim3(NTHR), 0, stream, wave, w0, N, k0, s0, C, T0, part);
    hipLaunchKernelGGL(m2f_w2v_conv0_merge_kernel, dim3((C + NTHR - 1) / NTHR, B), dim3(NTHR), 0, stream, part, nch, C, T0, eps, st);
    if (out16) {
        auto apply = m2f_w2v_conv0_apply_kernel<NT, true>;
        hipLaunchKernelGGL(apply, grid, dim3(NTHR), 0, stream, wave, w0, N, k0, s0, C, T0, P0, st, gamma, beta, nullptr, out16);
    } else {
        auto apply = m2f_w2v_conv0_apply_kernel<NT, false>;
        hipLaunchKernelGGL(apply, grid, dim3(NTHR), 0, stream, wave, w0, N, k0, s0, C, T0, P0, st, gamma, beta, out32, nullptr);
    }
}

}  // namespace

int m2f_w2v_conv0_chunks(int T0) { return (T0 + CONV0_FCH - 1) / CONV0_FCH; }

hipError_t m2f_launch_w2v_conv0(const float* wave, int B, int N, const float* w0, int k0, int s0, int C, int T0, int P0, const float* gamma,
                                const float* beta, float eps, float* partial, float* stats, float* out32, uint16_t* out16,
                                hipStream_t stream) {
    if (B < 1 || T0 < 1 || P0 < T0 || C < 1 || k0 < 1 || k0 > M2F_W2V_CONV0_MAX_TAPS || s0 < 1 || s0 > M2F_W2V_CONV0_MAX_STRIDE ||
        (T0 - 1) * s0 + k0 > N || !out32 == !out16)
        return hipErrorInvalidValue;
    const int nch = m2f_w2v_conv0_chunks(T0);
    float2* part = reinterpret_cast<float2*>(partial);
    float2* st = reinterpret_cast<float2*>(stats);
    const dim3 grid((P0 + CONV0_FCH - 1) / CONV0_FCH, B);
    if (k0 == 10) conv0_launch<10>(wave, B, N, w0, k0, s0, C, T0, P0, gamma, beta, eps, part, st, out32, out16, grid, nch, stream);   // (no zero taps)
    else conv0_launch<M2F_W2V_CONV0_MAX_TAPS>(wave, B, N, w0, k0, s0, C, T0, P0, gamma, beta, eps, part, st, out32, out16, grid, nch, stream);
    return hipGetLastError();
}

hipError_t m2f_launch_w2v_feat_ln(const float* x, int B, int S, int P, int C, const float* gamma, const float* beta, float eps, float* out32,
                                  uint16_t* out16, hipStream_t stream) {
    if (B < 1 || S < 1 || P < S || C < 1 || C > M2F_W2V_FEAT_MAX_C || !out32) return hipErrorInvalidValue;
    const int rpb = NTHR / 64;
    hipLaunchKernelGGL(m2f_w2v_feat_ln_kernel, dim3((B * S + rpb - 1) / rpb), dim3(NTHR), 0, stream, x, B, S, P, C, gamma, beta, eps, out32,
                       out16);
    return hipGetLastError();
}

size_t m2f_w2v_pos_conv_lds(int CG, int K, int bf16) {
    return (size_t)(PC_TILE + K - 1) * (CG + 4) * sizeof(float) + (size_t)PC_TAPS * CG * (CG + 4) * (bf16 ? 2 : 4);
}

hipError_t m2f_launch_w2v_pos_conv(const float* x, const int* lengths, int B, int S, int d, int groups, int K, const void* w, const float* bias,
                                   float* out, int bf16, hipStream_t stream) {
    if (B < 1 || S < 1 || groups < 1 || d % groups || K < 1 || K > M2F_W2V_POS_MAX_TAPS) return hipErrorInvalidValue;
    const int CG = d / groups;
    if (CG % 16 || CG > 64) return hipErrorInvalidValue;
    const size_t lds = m2f_w2v_pos_conv_lds(CG, K, bf16);
    const dim3 grid((S + PC_TILE - 1) / PC_TILE, groups, B);
#define M2F_PC_LAUNCH(NJ, BF)                                                                                                          \
    do {                                                                                                                               \
        auto kern = m2f_w2v_pos_conv_kernel<NJ, BF>;                                                                                   \
        if (lds > 64 * 1024) {                                                                                                         \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e;                                                                                             \
        }                                                                                                                              \
        hipLaunchKernelGGL(kern, grid, dim3(NTHR), lds, stream, x, lengths, w, bias, out, S, d, K);                                   \
    } while (0)
    switch (CG / 16 * 2 + (bf16 ? 1 : 0)) {
        case 2: M2F_PC_LAUNCH(1, false); break;
        case 3: M2F_PC_LAUNCH(1, true); break;
        case 4: M2F_PC_LAUNCH(2, false); break;
        case 5: M2F_PC_LAUNCH(2, true); break;
        case 6: M2F_PC_LAUNCH(3, false); break;
        case 7: M2F_PC_LAUNCH(3, true); break;
        case 8: M2F_PC_LAUNCH(4, false); break;
        case 9: M2F_PC_LAUNCH(4, true); break;
        default: return hipErrorInvalidValue;
    }
#undef M2F_PC_LAUNCH
    return hipGetLastError();
}

hipError_t m2f_launch_w2v_masked_mean(const float* x, const int* lengths, int B, int S, int d, float* out, hipStream_t stream) {
    if (B < 1 || S < 1 || d < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_w2v_masked_mean_kernel, dim3((d + NTHR - 1) / NTHR, B), dim3(NTHR), 0, stream, x, lengths, S, d, out);
    return hipGetLastError();
}
