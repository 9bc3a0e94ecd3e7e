// In-loop audio_mel encoder (mel_resnet.py): log-mel spectrogram front end, ResNet18 backbone and projection head on gfx950.
// Reference: src/feature_extractors/audio_mel (dataset.py _get_mel_spectrogram / get_mel_spectrogram, model.py, embeddings.py).
//
//   peak                      per utterance max |x| over the valid samples (order-free)
//   STFT + |.| + mel + log    per (utterance, 16-frame tile): the framed samples / peak in LDS, a windowed DFT against a cos/sin basis
//                             (fp32 FMA, 4 samples per LDS read), the magnitudes in LDS, the 128 mel rows, log(mel + eps)
//   normalise                 per utterance: exact min / max over the valid frames x 128 bands, (v - min) / (max - min), optional
//                             8-bit levels floor(v * 255) / 255, zero rows up to 1001 frames; peak 0 or max == min gives zeros
//   stem                      7x7/2 conv (the three identical channels and BatchNorm folded at pack time) + bias + ReLU + 3x3/2
//                             max pool, fp32 FMA in both precision modes; one workgroup = 4 pooled rows x 16 channels
//   convolution               implicit GEMM over NHWC activations (M = utterances x Ho x Wo, N = Cout, K = taps x Cin), every
//                             32-wide k-tile inside one tap, padding by predicated zero loads; BatchNorm folded into the weights
//                             and a bias; epilogue bias, optional residual, optional ReLU
//   head                      fixed-order average pool, fc 512 -> 1000 + bias, ReLU, 1000 -> 300 + bias, L2 normalise
//
// Nothing couples the utterances of a batch: every reduction runs inside one utterance in a fixed order, so an utterance's result
// does not depend on its batch partners.  No atomics.
#include <type_traits>

#include "common.h"
#include "ops.h"

namespace {

constexpr int NTHR = 256;

// ---- front end -----------------------------------------------------------------------------------------------------------------
constexpr int FE_FRAMES = 16;                                      // frames per STFT workgroup
constexpr int FE_SPAN = (FE_FRAMES - 1) * M2F_MEL_HOP + M2F_MEL_NFFT;
constexpr int FE_BINS = M2F_MEL_NFFT / 2 + 1;                      // 201
constexpr int FE_MP = FE_BINS + 3;                                 // magnitude row pitch in LDS

__global__ __launch_bounds__(NTHR) void m2f_mel_peak_kernel(const float* __restrict__ wave, const int* __restrict__ lengths, int N,
                                                             float* __restrict__ peak) {
    __shared__ float red[NTHR / 64];
    const int b = blockIdx.x;
    const int len = min(max(lengths[b], 0), N);
    const float* w = wave + (size_t)b * N;
    float m = 0.f;
    for (int i = threadIdx.x; i < len; i += NTHR) m = fmaxf(m, fabsf(w[i]));
    m = m2f_wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) peak[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// logmel[b][f][m] = log(sum_k fbT[k][m] |sum_t basis[t][k] y[f * hop - nfft/2 + t]| + eps) for f < frames(b); y = x / peak, zero
// outside the valid samples (centred frames, constant padding).  basis[t][0..200] = hann[t] cos(2 pi k t / nfft), [201..401] the sine.
__global__ __launch_bounds__(NTHR) void m2f_mel_stft_kernel(const float* __restrict__ wave, const int* __restrict__ lengths, int N,
                                                             const float* __restrict__ peak, const float* __restrict__ basis,
                                                             const float* __restrict__ fbT, float* __restrict__ logmel) {
    __shared__ __attribute__((aligned(16))) float xs[FE_SPAN];
    __shared__ float mag[FE_FRAMES * FE_MP];
    const int b = blockIdx.y, f0 = blockIdx.x * FE_FRAMES;
    const int len = min(max(lengths[b], 0), N);
    const int frames = min(1 + len / M2F_MEL_HOP, M2F_MEL_FRAMES);
    if (f0 >= frames) return;
    const float pk = peak[b];
    const float* w = wave + (size_t)b * N;
    const int s0 = f0 * M2F_MEL_HOP - M2F_MEL_NFFT / 2;
    for (int i = threadIdx.x; i < FE_SPAN; i += NTHR) {
        const int s = s0 + i;
        xs[i] = (s >= 0 && s < len && pk > 0.f) ? w[s] / pk : 0.f;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < FE_BINS) {
        float re[FE_FRAMES], im[FE_FRAMES];
#pragma unroll
        for (int f = 0; f < FE_FRAMES; ++f) re[f] = im[f] = 0.f;
        for (int t = 0; t < M2F_MEL_NFFT; t += 4) {
            float c[4], s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                c[u] = basis[(size_t)(t + u) * 2 * FE_BINS + k];
                s[u] = basis[(size_t)(t + u) * 2 * FE_BINS + FE_BINS + k];
            }
#pragma unroll
            for (int f = 0; f < FE_FRAMES; ++f) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(xs + f * M2F_MEL_HOP + t);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    re[f] = fmaf(c[u], x[u], re[f]);
                    im[f] = fmaf(s[u], x[u], im[f]);
                }
            }
        }
#pragma unroll
        for (int f = 0; f < FE_FRAMES; ++f) mag[f * FE_MP + k] = sqrtf(fmaf(re[f], re[f], im[f] * im[f]));
    }
    __syncthreads();
    const int m = threadIdx.x & (M2F_MEL_BANDS - 1), fh = threadIdx.x / M2F_MEL_BANDS;    // 2 halves of 8 frames
    constexpr int FH = FE_FRAMES / (NTHR / M2F_MEL_BANDS);
    float acc[FH];
#pragma unroll
    for (int i = 0; i < FH; ++i) acc[i] = 0.f;
    for (int kk = 0; kk < FE_BINS; ++kk) {
        const float wgt = fbT[kk * M2F_MEL_BANDS + m];
#pragma unroll
        for (int i = 0; i < FH; ++i) acc[i] = fmaf(wgt, mag[(fh * FH + i) * FE_MP + kk], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < FH; ++i) {
        const int f = f0 + fh * FH + i;
        if (f < frames) logmel[((size_t)b * M2F_MEL_FRAMES + f) * M2F_MEL_BANDS + m] = logf(acc[i] + M2F_MEL_LOG_EPS);
    }
}

// img[b] = the stem's input: (v - min) / (max - min) over the valid frames (8-bit levels when `levels`), zero rows behind them
__global__ __launch_bounds__(NTHR) void m2f_mel_norm_kernel(const float* __restrict__ logmel, const int* __restrict__ lengths, int N,
                                                             const float* __restrict__ peak, int levels, float* __restrict__ img) {
    __shared__ float red[2][NTHR / 64];
    const int b = blockIdx.x;
    const int len = min(max(lengths[b], 0), N);
    const int n = min(1 + len / M2F_MEL_HOP, M2F_MEL_FRAMES) * M2F_MEL_BANDS;
    const float* src = logmel + (size_t)b * M2F_MEL_FRAMES * M2F_MEL_BANDS;
    float* dst = img + (size_t)b * M2F_MEL_FRAMES * M2F_MEL_BANDS;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < n; i += NTHR) {
        const float v = src[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = -m2f_wave_max(-lo);
    hi = m2f_wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    const bool flat = !(peak[b] > 0.f) || !(hi > lo);              // the reference divides by zero here: defined as an all-zero image
    const float range = hi - lo;
    for (int i = threadIdx.x; i < M2F_MEL_FRAMES * M2F_MEL_BANDS; i += NTHR) {
        float v = 0.f;
        if (i < n && !flat) {
            v = (src[i] - lo) / range;
            if (levels) v = floorf(v * 255.f) / 255.f;
        }
        dst[i] = v;
    }
}

// ---- stem: 7x7/2 conv (one folded input channel) + bias + ReLU + 3x3/2 max pool, pad 3 / pad 1 -----------------------------------
constexpr int ST_PR = 4;                                           // pooled rows per workgroup
constexpr int ST_CG = 16;                                          // output channels per workgroup
constexpr int ST_SR = 2 * ST_PR + 1;                               // stem rows it needs
constexpr int ST_IR = 2 * ST_SR + 5;                               // input rows it needs
constexpr int ST_IC = 2 * M2F_MEL_STEM_W + 5;                      // input columns incl. the padding (-3 .. 2 * 63 + 3)
constexpr int ST_ICP = ST_IC + 3;

template <bool OUT16>
__global__ __launch_bounds__(NTHR) void m2f_mel_stem_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ out32,
                                                             uint16_t* __restrict__ out16) {
    __shared__ float xs[ST_IR * ST_ICP];
    __shared__ __attribute__((aligned(16))) float ws[49 * ST_CG];
    __shared__ __attribute__((aligned(16))) float st[ST_SR * M2F_MEL_STEM_W * ST_CG];
    const int p0 = blockIdx.x * ST_PR, g = blockIdx.y, b = blockIdx.z;
    const int r0 = 2 * p0 - 1, i0 = 2 * r0 - 3;                     // first stem row, first input row
    const float* src = img + (size_t)b * M2F_MEL_FRAMES * M2F_MEL_BANDS;
    for (int i = threadIdx.x; i < ST_IR * ST_IC; i += NTHR) {
        const int r = i / ST_IC, c = i - r * ST_IC, ir = i0 + r, ic = c - 3;
        xs[r * ST_ICP + c] = (ir >= 0 && ir < M2F_MEL_FRAMES && ic >= 0 && ic < M2F_MEL_BANDS) ? src[ir * M2F_MEL_BANDS + ic] : 0.f;
    }
    for (int i = threadIdx.x; i < 49 * ST_CG; i += NTHR) ws[i] = w[(i / ST_CG) * M2F_MEL_C0 + g * ST_CG + (i % ST_CG)];
    __syncthreads();
    for (int it = threadIdx.x; it < ST_SR * M2F_MEL_STEM_W; it += NTHR) {
        asm volatile("" ::: "memory");                             // (keeps the weight reads in the loop: hoisted, they spill)
        const int rr = it / M2F_MEL_STEM_W, wc = it - rr * M2F_MEL_STEM_W, r = r0 + rr;
        f32x4 acc[ST_CG / 4];
#pragma unroll
        for (int q = 0; q < ST_CG / 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r >= 0 && r < M2F_MEL_STEM_H) {
#pragma unroll 1
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    const float x = xs[(2 * rr + i) * ST_ICP + 2 * wc + j];
                    const f32x4* wr = reinterpret_cast<const f32x4*>(ws + (i * 7 + j) * ST_CG);
#pragma unroll
                    for (int q = 0; q < ST_CG / 4; ++q) acc[q] += x * wr[q];
                }
            }
#pragma unroll
            for (int q = 0; q < ST_CG / 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[q][e] = fmaxf(acc[q][e] + bias[g * ST_CG + 4 * q + e], 0.f);
        }
        // (rows outside the stem read as 0: every pool window holds a valid row, and ReLU outputs are >= 0)
        f32x4* d = reinterpret_cast<f32x4*>(st + it * ST_CG);
#pragma unroll
        for (int q = 0; q < ST_CG / 4; ++q) d[q] = acc[q];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < ST_PR * M2F_MEL_POOL_W * ST_CG; it += NTHR) {
        const int c = it % ST_CG, q = (it / ST_CG) % M2F_MEL_POOL_W, pr = it / (ST_CG * M2F_MEL_POOL_W), p = p0 + pr;
        if (p >= M2F_MEL_POOL_H) continue;
        float m = 0.f;
#pragma unroll
        for (int dr = 0; dr < 3; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) {
                const int sc = 2 * q + dc;
                if (sc >= 0 && sc < M2F_MEL_STEM_W) m = fmaxf(m, st[((2 * pr + dr) * M2F_MEL_STEM_W + sc) * ST_CG + c]);
            }
        const size_t o = (((size_t)b * M2F_MEL_POOL_H + p) * M2F_MEL_POOL_W + q) * M2F_MEL_C0 + g * ST_CG + c;
        if constexpr (OUT16) out16[o] = m2f_bf16_bits(m);
        else out32[o] = m;
    }
}

// ---- implicit-GEMM convolution, NHWC ---------------------------------------------------------------------------------------------
// out[m][n] = act(sum_{tap, c} x[b][ho*s - pad + dy][wo*s - pad + dx][c] * w[n][tap][c] + bias[n] (+ res[m][n])), m = (b*Ho + ho)*Wo + wo.
// Workgroup tile 128 (M) x 64 (N), four waves 2 x 2 of 64 x 32, k-tiles of 32 input channels of one tap.  Operand tiles are loaded
// global -> registers one k-tile ahead and stored to the other of two LDS buffers (one barrier per k-tile).  bf16: 16x16x32 bf16
// MFMA (one per 16 x 16 sub-tile and k-tile); fp32: 16x16x4 fp32 MFMA (eight).
constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 32;

template <bool BF16>
struct ConvT {
    typedef typename std::conditional<BF16, uint16_t, float>::type T;
    static constexpr int PITCH = BF16 ? CV_BK + 8 : CV_BK + 4;     // LDS row pitch in elements (16-B aligned, spreads the banks)
    static constexpr int EPC = 16 / sizeof(T);                     // elements per 16-B chunk
    static constexpr int CPR = CV_BK / EPC;                        // chunks per row
    static constexpr int A_CH = CV_BM * CPR / NTHR;                // A chunks per thread
    static constexpr int B_CH = CV_BN * CPR / NTHR;
};

template <bool BF16, bool OUT16>
__global__ __launch_bounds__(NTHR) void m2f_mel_conv_kernel(const void* __restrict__ xv, const void* __restrict__ wv,
                                                             const float* __restrict__ bias, const void* __restrict__ resv,
                                                             void* __restrict__ outv, int M, int H, int W, int Cin, int Ho, int Wo,
                                                             int Cout, int ks, int stride, int relu) {
    typedef ConvT<BF16> CT;
    typedef typename CT::T T;
    constexpr int P = CT::PITCH, EPC = CT::EPC, CPR = CT::CPR;
    __shared__ __attribute__((aligned(16))) T As[2][CV_BM * P];
    __shared__ __attribute__((aligned(16))) T Bs[2][CV_BN * P];
    const T* x = reinterpret_cast<const T*>(xv);
    const T* w = reinterpret_cast<const T*>(wv);
    const int tid = threadIdx.x, lane = tid & 63, wvi = tid >> 6, wm = wvi >> 1, wn = wvi & 1, l16 = lane & 15, lq = lane >> 4;
    const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
    const int pad = ks / 2, K = ks * ks * Cin, cpt = Cin / CV_BK, nk = ks * ks * cpt;

    // this thread's A rows: the input pixel of tap (0, 0) and the image base, fixed over the k loop
    int a_ih[CT::A_CH], a_iw[CT::A_CH];
    int64_t a_base[CT::A_CH];
#pragma unroll
    for (int j = 0; j < CT::A_CH; ++j) {
        const int m = m0 + (tid + j * NTHR) / CPR;
        if (m < M) {
            const int b = m / (Ho * Wo), rem = m - b * Ho * Wo, ho = rem / Wo, wo = rem - ho * Wo;
            a_ih[j] = ho * stride - pad;
            a_iw[j] = wo * stride - pad;
            a_base[j] = (int64_t)b * H * W;
        } else {
            a_ih[j] = -(1 << 20);                                   // never valid
            a_iw[j] = 0;
            a_base[j] = 0;
        }
    }
    f32x4 ra[CT::A_CH], rb[CT::B_CH];
    auto load = [&](int kt) {
        const int tap = kt / cpt, c0 = (kt - tap * cpt) * CV_BK, dy = tap / ks, dx = tap - dy * ks;
#pragma unroll
        for (int j = 0; j < CT::A_CH; ++j) {
            const int cc = ((tid + j * NTHR) % CPR) * EPC;
            const int ih = a_ih[j] + dy, iw = a_iw[j] + dx;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W)
                ra[j] = *reinterpret_cast<const f32x4*>(x + ((a_base[j] + (int64_t)ih * W + iw) * Cin + c0 + cc));
            else
                ra[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < CT::B_CH; ++j) {
            const int i = tid + j * NTHR, n = i / CPR, cc = (i % CPR) * EPC;
            rb[j] = *reinterpret_cast<const f32x4*>(w + ((int64_t)(n0 + n) * K + (int64_t)kt * CV_BK + cc));
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < CT::A_CH; ++j) {
            const int i = tid + j * NTHR;
            *reinterpret_cast<f32x4*>(&As[buf][(i / CPR) * P + (i % CPR) * EPC]) = ra[j];
        }
#pragma unroll
        for (int j = 0; j < CT::B_CH; ++j) {
            const int i = tid + j * NTHR;
            *reinterpret_cast<f32x4*>(&Bs[buf][(i / CPR) * P + (i % CPR) * EPC]) = rb[j];
        }
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load(kt + 1);
        const T* as = As[buf] + (wm * 64 + l16) * P;
        const T* bs = Bs[buf] + (wn * 32 + l16) * P;
        if constexpr (BF16) {
            bf16x8 a[4], bb[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(as + i * 16 * P + 8 * lq);
#pragma unroll
            for (int j = 0; j < 2; ++j) bb[j] = *reinterpret_cast<const bf16x8*>(bs + j * 16 * P + 8 * lq);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bb[j], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int k4 = 0; k4 < CV_BK; k4 += 4) {
                float a[4], bb[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = as[i * 16 * P + k4 + lq];
#pragma unroll
                for (int j = 0; j < 2; ++j) bb[j] = bs[j * 16 * P + k4 + lq];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bb[j], acc[i][j], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) store(buf ^ 1);
        __syncthreads();
    }

    // accumulator element r of sub-tile (i, j): row m0 + 64 wm + 16 i + 4 lq + r, column n0 + 32 wn + 16 j + l16
    const T* res = reinterpret_cast<const T*>(resv);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn * 32 + j * 16 + l16;
        const float bn = bias[n];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 64 + i * 16 + 4 * lq + r;
                if (m >= M) continue;
                const size_t o = (size_t)m * Cout + n;
                float v = acc[i][j][r] + bn;
                if (res) {
                    if constexpr (BF16) v += m2f_bf16_to_f32(res[o]);
                    else v += res[o];
                }
                if (relu) v = fmaxf(v, 0.f);
                if constexpr (OUT16) reinterpret_cast<uint16_t*>(outv)[o] = m2f_bf16_bits(v);
                else reinterpret_cast<float*>(outv)[o] = v;
            }
    }
}

// ---- head ------------------------------------------------------------------------------------------------------------------------
// per utterance: pooled = mean over HW positions (fixed order), h = ReLU(pooled W1^T + b1), e = h W2^T + b2, e / max(|e|, 1e-12).
// (torchvision's fc output goes through the projector's ReLU; w1t [C][N1] and w2t [N1][N2] are the transposed weights.)
constexpr int HD_UB = 1;                                           // utterances per workgroup (more share the weight reads, but at 8 the
                                                                   // 64-utterance batch ran on 8 workgroups: 1.5 ms)

template <bool IN16>
__global__ __launch_bounds__(NTHR) void m2f_mel_head_kernel(const void* __restrict__ xv, int B, int HW, int C,
                                                             const float* __restrict__ w1t, const float* __restrict__ b1, int N1,
                                                             const float* __restrict__ w2t, const float* __restrict__ b2, int N2,
                                                             float* __restrict__ out) {
    extern __shared__ float sm[];
    float* pooled = sm;                                            // [HD_UB][C]
    float* hid = sm + HD_UB * C;                                   // [HD_UB][N1]
    __shared__ float red[HD_UB][NTHR / 64];
    const int u0 = blockIdx.x * HD_UB, nu = min(HD_UB, B - u0);
    for (int i = threadIdx.x; i < HD_UB * C; i += NTHR) {
        const int u = i / C, c = i - u * C;
        float s = 0.f;
        if (u < nu) {
            const size_t base = (size_t)(u0 + u) * HW * C + c;
            for (int p = 0; p < HW; ++p) {
                if constexpr (IN16) s += m2f_bf16_to_f32(reinterpret_cast<const uint16_t*>(xv)[base + (size_t)p * C]);
                else s += reinterpret_cast<const float*>(xv)[base + (size_t)p * C];
            }
        }
        pooled[i] = s / (float)HW;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < N1; o += NTHR) {
        float a[HD_UB];
#pragma unroll
        for (int u = 0; u < HD_UB; ++u) a[u] = 0.f;
        for (int c = 0; c < C; ++c) {
            const float wgt = w1t[(size_t)c * N1 + o];
#pragma unroll
            for (int u = 0; u < HD_UB; ++u) a[u] = fmaf(pooled[u * C + c], wgt, a[u]);
        }
#pragma unroll
        for (int u = 0; u < HD_UB; ++u) hid[u * N1 + o] = fmaxf(a[u] + b1[o], 0.f);
    }
    __syncthreads();
    float e[HD_UB][2];
    float ss[HD_UB];
#pragma unroll
    for (int u = 0; u < HD_UB; ++u) ss[u] = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int o = threadIdx.x + q * NTHR;
        float a[HD_UB];
#pragma unroll
        for (int u = 0; u < HD_UB; ++u) a[u] = 0.f;
        if (o < N2) {
            for (int c = 0; c < N1; ++c) {
                const float wgt = w2t[(size_t)c * N2 + o];
#pragma unroll
                for (int u = 0; u < HD_UB; ++u) a[u] = fmaf(hid[u * N1 + c], wgt, a[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < HD_UB; ++u) {
            e[u][q] = o < N2 ? a[u] + b2[o] : 0.f;
            ss[u] = fmaf(e[u][q], e[u][q], ss[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < HD_UB; ++u) {
        const float s = m2f_wave_sum(ss[u]);
        if ((threadIdx.x & 63) == 0) red[u][threadIdx.x >> 6] = s;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < HD_UB; ++u) {
        if (u >= nu) continue;
        const float nrm = sqrtf((red[u][0] + red[u][1]) + (red[u][2] + red[u][3]));
        const float inv = 1.f / fmaxf(nrm, 1e-12f);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o = threadIdx.x + q * NTHR;
            if (o < N2) out[(size_t)(u0 + u) * N2 + o] = e[u][q] * inv;
        }
    }
}

}  // namespace

hipError_t m2f_launch_mel_frontend(const float* wave, const int* lengths, int B, int N, const float* basis, const float* fbT, int levels,
                                   float* peak, float* logmel, float* img, hipStream_t stream) {
    if (B < 1 || N < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_mel_peak_kernel, dim3(B), dim3(NTHR), 0, stream, wave, lengths, N, peak);
    hipLaunchKernelGGL(m2f_mel_stft_kernel, dim3((M2F_MEL_FRAMES + FE_FRAMES - 1) / FE_FRAMES, B), dim3(NTHR), 0, stream, wave, lengths, N,
                       peak, basis, fbT, logmel);
    hipLaunchKernelGGL(m2f_mel_norm_kernel, dim3(B), dim3(NTHR), 0, stream, logmel, lengths, N, peak, levels, img);
    return hipGetLastError();
}

hipError_t m2f_launch_mel_stem(const float* img, int B, const float* w, const float* bias, float* out32, uint16_t* out16,
                               hipStream_t stream) {
    if (B < 1 || !out32 == !out16) return hipErrorInvalidValue;
    const dim3 grid((M2F_MEL_POOL_H + ST_PR - 1) / ST_PR, M2F_MEL_C0 / ST_CG, B);
    if (out16) hipLaunchKernelGGL(m2f_mel_stem_kernel<true>, grid, dim3(NTHR), 0, stream, img, w, bias, nullptr, out16);
    else hipLaunchKernelGGL(m2f_mel_stem_kernel<false>, grid, dim3(NTHR), 0, stream, img, w, bias, out32, nullptr);
    return hipGetLastError();
}

hipError_t m2f_launch_mel_conv(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int H, int W, int Cin,
                               int Cout, int ks, int stride, int bf16, int out32, int relu, hipStream_t stream) {
    if (B < 1 || H < 1 || W < 1 || Cin % CV_BK || Cin < CV_BK || Cout % CV_BN || Cout < CV_BN || (ks != 1 && ks != 3) || stride < 1)
        return hipErrorInvalidValue;
    const int pad = ks / 2, Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const int64_t M64 = (int64_t)B * Ho * Wo;
    if (Ho < 1 || Wo < 1 || M64 > (1 << 30)) return hipErrorInvalidValue;
    const int M = (int)M64;
    const dim3 grid((M + CV_BM - 1) / CV_BM, Cout / CV_BN);
    if (bf16 && !out32)
        hipLaunchKernelGGL((m2f_mel_conv_kernel<true, true>), grid, dim3(NTHR), 0, stream, x, w, bias, res, out, M, H, W, Cin, Ho, Wo, Cout, ks,
                           stride, relu);
    else if (bf16)
        hipLaunchKernelGGL((m2f_mel_conv_kernel<true, false>), grid, dim3(NTHR), 0, stream, x, w, bias, res, out, M, H, W, Cin, Ho, Wo, Cout,
                           ks, stride, relu);
    else
        hipLaunchKernelGGL((m2f_mel_conv_kernel<false, false>), grid, dim3(NTHR), 0, stream, x, w, bias, res, out, M, H, W, Cin, Ho, Wo,
                           Cout, ks, stride, relu);
    return hipGetLastError();
}

hipError_t m2f_launch_mel_head(const void* x, int in16, int B, int HW, int C, const float* w1t, const float* b1, int N1, const float* w2t,
                               const float* b2, int N2, float* out, hipStream_t stream) {
    if (B < 1 || HW < 1 || C < 1 || N1 < 1 || N2 < 1 || N2 > 2 * NTHR) return hipErrorInvalidValue;
    const size_t lds = (size_t)HD_UB * (C + N1) * sizeof(float);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const dim3 grid((B + HD_UB - 1) / HD_UB);
    if (in16) hipLaunchKernelGGL(m2f_mel_head_kernel<true>, grid, dim3(NTHR), lds, stream, x, B, HW, C, w1t, b1, N1, w2t, b2, N2, out);
    else hipLaunchKernelGGL(m2f_mel_head_kernel<false>, grid, dim3(NTHR), lds, stream, x, B, HW, C, w1t, b1, N1, w2t, b2, N2, out);
    return hipGetLastError();
}
