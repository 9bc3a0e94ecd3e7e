// Shared device helpers for the M2FNet gfx950 kernels (wave64, MFMA, LDS).
// gfx950 only: no CUDA shims, no alternate back-ends.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// Kernel-argument warm-up.  The kernels take their launch descriptors (GemmBatch, AttnBatch, LnBatch: 0.5-3 KB) BY VALUE; the
// kernarg segment of a launch is cold in the scalar cache and in L2, and hipcc issues its s_loads lazily - a grouped GEMM
// prologue walked four DEPENDENT misses (hidden grid size -> total_tiles -> tb[] -> hot[pi]) before its first operand load.
// One wave-wide batch of s_load_dword, one per 64-byte line the kernel is going to read, turns them into one miss + hits.
// (The wait sits INSIDE the asm: the compiler does not track loads issued by inline asm, and the scratch register is dead
// the moment the block ends.)
#define M2F_KW1(op, i) "s_load_dword %0, %1, " op "+(" #i ")*64\n"
#define M2F_KW8(op, b) M2F_KW1(op, b+0) M2F_KW1(op, b+1) M2F_KW1(op, b+2) M2F_KW1(op, b+3) M2F_KW1(op, b+4) M2F_KW1(op, b+5) M2F_KW1(op, b+6) M2F_KW1(op, b+7)
// LINES (8, 16 or 24) consecutive 64-byte lines from byte offset B on, plus eight more from B2 on (B2 < 0: none; the hidden
// arguments behind a large struct); every load writes the same scratch register.
template <int B, int LINES = 8, int B2 = -1>
__device__ __forceinline__ void m2f_kernarg_warm() {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(M2F_NO_KERNARG_WARM)       // (the switch exists for A/B builds)
    static_assert(B % 4 == 0 && (B2 < 0 || B2 % 4 == 0) && (LINES == 8 || LINES == 16 || LINES == 24), "dword offsets, whole groups of eight lines");
    const auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    constexpr int C = B2 < 0 ? B : B2;          // (no second range: its loads repeat the first lines - hits)
    uint32_t t;
    if constexpr (LINES == 8) asm volatile(M2F_KW8("%2", 0) M2F_KW8("%3", 0) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(kp), "n"(B), "n"(C) : "memory");
    else if constexpr (LINES == 16) asm volatile(M2F_KW8("%2", 0) M2F_KW8("%2", 8) M2F_KW8("%3", 0) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(kp), "n"(B), "n"(C) : "memory");
    else asm volatile(M2F_KW8("%2", 0) M2F_KW8("%2", 8) M2F_KW8("%2", 16) M2F_KW8("%3", 0) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(kp), "n"(B), "n"(C) : "memory");
#endif
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define M2F_WAVE 64

// ---- counter-based dropout RNG -----------------------------------------------------------------
// The state lives in device memory (4 x u32: seed_lo, seed_hi, step_lo, step_hi) so a captured
// hipGraph replays with a fresh stream of masks each step (a 1-thread kernel bumps `step`).
// keep(site, idx) is a pure function of (state, site, idx): the backward pass regenerates the
// forward mask instead of storing it.
__device__ __forceinline__ uint32_t m2f_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// the site key from the four state words already in registers (m2f_rng_words below): the one statement of the key's arithmetic
__device__ __forceinline__ uint32_t m2f_site_key_words(u32x4 w, uint32_t site) {
    uint32_t k = m2f_mix32(w[0] ^ 0x9e3779b9U);
    k = m2f_mix32(k ^ w[1]);
    k = m2f_mix32(k + w[2] * 0x85ebca6bU);
    k = m2f_mix32(k ^ (w[3] + site * 0xc2b2ae35U));
    return k;
}
__device__ __forceinline__ uint32_t m2f_site_key(const uint32_t* __restrict__ rng, uint32_t site) {
    const u32x4 w = {rng[0], rng[1], rng[2], rng[3]};
    return m2f_site_key_words(w, site);
}
__device__ __forceinline__ bool m2f_keep(uint32_t key, uint32_t idx, uint32_t thresh) {
    uint32_t h = m2f_mix32(idx * 0x9E3779B1U + key);
    h = m2f_mix32(h ^ (key >> 7) ^ 0x68e31da4U);
    return h >= thresh;       // P(keep) = 1 - thresh / 2^32
}

// ---- range-checked buffer loads ------------------------------------------------------------------
// A load the row-wise kernels may or may not need (a nullable operand, a chunk behind the row's end, the dropout state) is
// issued UNCONDITIONALLY through a buffer descriptor of `bytes` bytes at `p` (0 bytes for a null `p`): what lies outside reads as
// zero and touches no memory.  A guarded plain load instead (`if (p) x = *p`, `if (c < d) ...`) compiles to a branch whose join
// waits for every outstanding load, one memory round trip per guard (see rowops.hip).  `p` and `bytes` must be wave-uniform.
typedef __amdgpu_buffer_rsrc_t m2f_rsrc_t;
__device__ __forceinline__ m2f_rsrc_t m2f_make_rsrc(const void* p, uint32_t bytes) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane(p ? (int)bytes : 0), 0x00020000);
}
// ---- result stores through a buffer descriptor: plain (L2 write-back) or write-through ----------------
// WT = true sets the descriptor store's cache-policy operand to 16: on gfx950 `buffer_store_dwordx4 ... offen sc1`, the
// write-through form - the bytes leave the XCD's L2 while the kernel still runs instead of at the release that ends it.  WT =
// false emits the plain form of the same instruction.  Never `nt`.  `off` is the byte offset into the descriptor's range; a store
// outside the range is dropped.  Which kernel family writes through is a compile-time choice (M2F_WT_RING, M2F_WT_ROWS,
// M2F_WT_ATTN below, 1 or 0): no runtime flag, no second instantiation.  No fence or wait goes with these stores: every wave
// drains its own at s_endpgm and visibility across launches stays the kernel boundary's.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <bool WT>
__device__ __forceinline__ void m2f_store_b128(m2f_rsrc_t rs, uint32_t off, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (int)off, 0, WT ? 16 : 0);
}
template <bool WT>
__device__ __forceinline__ void m2f_store_b64(m2f_rsrc_t rs, uint32_t off, uint32_t lo, uint32_t hi) {
    const u32x2 w = {lo, hi};
    __builtin_amdgcn_raw_buffer_store_b64(w, rs, (int)off, 0, WT ? 16 : 0);
}
template <bool WT>
__device__ __forceinline__ void m2f_store_b32(m2f_rsrc_t rs, uint32_t off, uint32_t w) {
    __builtin_amdgcn_raw_buffer_store_b32(w, rs, (int)off, 0, WT ? 16 : 0);
}
// Which families write their results through: the ones that passed the A/B on the C3 bf16 step.  The
// LayerNorm kernels do (-0.044 ms per step).  The ring epilogue's fp32 C stores (-0.018 ms) and the one-tile attention kernels'
// (-0.016 ms) were faster in every alternated run but by less than three times the runs' own spread: measured, not kept, off.
// `make wt_flip_ring / wt_flip_rows / wt_flip_attn` build the library with ONE family's switch turned over, for the next A/B.
#ifndef M2F_WT_RING
#define M2F_WT_RING 0
#endif
#ifndef M2F_WT_ROWS
#define M2F_WT_ROWS 1
#endif
#ifndef M2F_WT_ATTN
#define M2F_WT_ATTN 0
#endif

// the dropout state (seed_lo, seed_hi, step_lo, step_hi) as one 16-byte load in flight with the caller's other loads; zeros for a
// null `rng` (a launch without a dropout site)
__device__ __forceinline__ u32x4 m2f_rng_words(const uint32_t* rng) {
    return __builtin_amdgcn_raw_buffer_load_b128(m2f_make_rsrc(rng, 16), 0, 0, 0);
}
// Left alone, hipcc sinks that load into the `if (site)` that uses it - behind the other loads' wait, a round trip of its own.  An
// (empty) unconditional use keeps it where the source issues it; place the use where the words have certainly arrived (behind a
// wait for loads issued AFTER them: the vector memory counter retires loads in order), so that it costs no wait itself.
__device__ __forceinline__ void m2f_rng_words_arrived(u32x4& w) { asm volatile("" : "+v"(w)); }

// Focal factor (1 - p_y)^gamma of a criterion row (criterion_row.h's focal part, behind rowops.hip m2f_ce_focal_kernel and metrics.hip
// m2f_eval_rows_kernel<true>: ONE function, so the eval loss has the train criterion's bits).  omp is the SUM of the other classes' probabilities, never 1 - p_y.  gamma == 0 SELECTS 1;
// omp == 0 (the other classes' expf underflowed) selects 0 for gamma > 0: powf never sees a zero base, nothing computes 0 * anything.
__device__ __forceinline__ float m2f_focal_factor(float omp, float gamma) {
    return gamma > 0.f ? (omp > 0.f ? powf(omp, gamma) : 0.f) : 1.f;
}

__device__ __forceinline__ float m2f_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float m2f_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The ONE fixed-order sum of per-row terms by a workgroup of 256 (the criterion's finalize, the R-Drop KL reduce, the eval finalize: the
// eval loss has the train loss's bits because all three call this).  s[j] = sum over t of terms[N * t + j]: thread-strided over t,
// wave sum, the four waves' partials through LDS, (s0 + s1) + (s2 + s3); every thread gets the sums.  Holds one __syncthreads():
// all 256 threads call it, once per kernel.
template <int N>
__device__ __forceinline__ void m2f_block_sum_terms(const float* __restrict__ terms, int T, float (&s)[N]) {
    __shared__ float part[N][4];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) {
#pragma unroll
        for (int j = 0; j < N; ++j) s[j] += terms[N * t + j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        s[j] = m2f_wave_sum(s[j]);
        if ((threadIdx.x & 63) == 0) part[j][threadIdx.x >> 6] = s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = (part[j][0] + part[j][1]) + (part[j][2] + part[j][3]);
}

static inline int m2f_cdiv(int a, int b) { return (a + b - 1) / b; }

// Host-side pick among the instantiations of a kernel template: m2f_pick_bools(f, a, b, ...) calls f(std::bool_constant<a>{},
// std::bool_constant<b>{}, ...) for the runtime bools a, b, ... - every combination is instantiated, so a launcher names its kernel
// template once and a new flag is one more argument, never one more arm.
template <typename F>
auto m2f_pick_bools(F&& f) { return f(); }
template <typename F, typename... Rest>
auto m2f_pick_bools(F&& f, bool first, Rest... rest) {
    return first ? m2f_pick_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
                 : m2f_pick_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// fp32 -> bf16 bits, round to nearest even (same rounding the GEMM staging applies; NaN stays NaN)
__device__ __forceinline__ uint16_t m2f_bf16_bits(float x) {
    const __bf16 h = (__bf16)x;
    return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float m2f_bf16_to_f32(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }

// fp32 -> OCP e4m3 byte, saturating at +-448 (the value range the fp8 GEMM operands use)
__device__ __forceinline__ uint32_t m2f_fp8x4_bits(float a, float b, float c, float d) {
    a = fminf(fmaxf(a, -448.f), 448.f); b = fminf(fmaxf(b, -448.f), 448.f);
    c = fminf(fmaxf(c, -448.f), 448.f); d = fminf(fmaxf(d, -448.f), 448.f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);     // bytes 0, 1
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);      // bytes 2, 3
    return (uint32_t)w;
}

#ifdef __HIPCC__
// erf for the GELU epilogues.  POLY (bf16 / fp8 kernels): odd degree-13 minimax polynomial on |z| <= 3, max error 4.33e-4
// (far inside bf16 operand rounding), 7 FMAs, no quarter-rate instructions; otherwise Abramowitz-Stegun 7.1.26 (1.5e-7) on
// the hardware exp / rcp (libm's erff is several times slower still).
template <bool POLY>
__device__ __forceinline__ float m2f_gelu(float x) {
    const float z = x * 0.70710678118654752f;
    float e;
    if constexpr (POLY) {
        const float zc = fminf(fmaxf(z, -3.0f), 3.0f), t = zc * zc;
        float p = 3.4737140595098026e-06f;
        p = p * t - 0.0001298444258281961f;
        p = p * t + 0.0020486447028815746f;
        p = p * t - 0.018010087311267853f;
        p = p * t + 0.098881796002388f;
        p = p * t - 0.3658691942691803f;
        p = p * t + 1.1261212825775146f;
        e = fminf(fmaxf(p * zc, -1.0f), 1.0f);
    } else {
        const float az = fabsf(z);
        const float tt = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
        const float poly = tt * (0.254829592f + tt * (-0.284496736f + tt * (1.421413741f + tt * (-1.453152027f + tt * 1.061405429f))));
        e = copysignf(1.0f - poly * __expf(-az * az), z);
    }
    return 0.5f * x * (1.0f + e);
}
#endif
