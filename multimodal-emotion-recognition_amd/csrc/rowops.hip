// Row-wise (HBM-bound) kernels of the M2FNet step for gfx950: LayerNorm forward/backward with fused
// residual / dropout, the label-smoothed cross-entropy criterion (reference src/train.py:48-50) and the
// dropout-mask re-application used in backward.  (The fused optimizer is adam.hip.)
// One wavefront per token row, rows cached in registers, 16-byte coalesced accesses, wave shuffles for
// the row reductions; column reductions (dgamma/dbeta) go through per-block partials (deterministic,
// no atomics, no memset).
// The LayerNorm kernels' 16-byte path issues EVERY load of a wave - gamma, beta, x, residual / dy, extra, the row's statistics,
// the dropout state - in one batch of range-checked buffer loads (common.h) before the first wait, and waits with counted
// vmcnt: one memory round trip per wave.  (With a guard around every chunk, `if (c < d) { if (vec) ... }`, hipcc joined the
// arms behind a full `s_waitcnt vmcnt(0)` each: the backward kernel walked eight round trips before its first multiply, four of
// them for one row of gamma.)  The general path (d % 4 != 0 or an unaligned operand) keeps the guarded element loads.
#include "common.h"
#include "ops.h"
#include "criterion_row.h"
#include "param_walk.h"
#include <algorithm>

// No floating-point contraction in this file: several kernels restate the same formulas in different surroundings (ring and
// register-staged GEMM epilogues, fp32 and bf16 attention forms), and with -ffp-contract=fast (the
// HIP default) the compiler is free to fuse a*b+c in one of them and not in the other - a 1-ulp difference that would break the
// bit-for-bit comparisons the tests make between the forms.  These kernels are bound by memory or by MFMA, not by VALU multiplies.
#pragma clang fp contract(off)

namespace {

constexpr int LN_MAXV_LIMIT = 8;           // float4 chunks per lane  -> d <= 2048 (kernels templated on NV)
constexpr int LN_WAVES = 4;
constexpr int LN_ROWS_PER_WAVE = M2F_LN_ROWS_PER_BLOCK / LN_WAVES;

template <int NV> struct RowRegs { f32x4 v[NV]; };

// lane owns elements c = 4*(lane + 64*j) .. +3 ; scalar tail handling when d % 4 != 0 or unaligned.
template <int NV>
__device__ __forceinline__ void row_load(RowRegs<NV>& r, const float* __restrict__ p, int d, bool vec, int lane) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = 4 * (lane + 64 * j);
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (c < d) {
            if (vec) x = *reinterpret_cast<const f32x4*>(p + c);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < d) x[e] = p[c + e];
            }
        }
        r.v[j] = x;
    }
}
template <int NV>
__device__ __forceinline__ void row_store(const RowRegs<NV>& r, float* __restrict__ p, int d, bool vec, int lane) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = 4 * (lane + 64 * j);
        if (c < d) {
            if (vec) *reinterpret_cast<f32x4*>(p + c) = r.v[j];
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (c + e < d) p[c + e] = r.v[j][e];
            }
        }
    }
}
// bf16 shadow of a row (rows of shadowed buffers are 16-byte aligned in fp32, hence 8-byte aligned in bf16)
template <int NV>
__device__ __forceinline__ void row_store_bf16(const RowRegs<NV>& r, uint16_t* __restrict__ q, int d, int lane) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = 4 * (lane + 64 * j);
        if (c + 3 < d) {
            uint2 w;
            w.x = (uint32_t)m2f_bf16_bits(r.v[j][0]) | ((uint32_t)m2f_bf16_bits(r.v[j][1]) << 16);
            w.y = (uint32_t)m2f_bf16_bits(r.v[j][2]) | ((uint32_t)m2f_bf16_bits(r.v[j][3]) << 16);
            if ((reinterpret_cast<uintptr_t>(q + c) & 7) == 0) *reinterpret_cast<uint2*>(q + c) = w;
            else { q[c] = (uint16_t)w.x; q[c + 1] = (uint16_t)(w.x >> 16); q[c + 2] = (uint16_t)w.y; q[c + 3] = (uint16_t)(w.y >> 16); }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (c + e < d) q[c + e] = m2f_bf16_bits(r.v[j][e]);
        }
    }
}
__device__ __forceinline__ bool is_vec(const void* p, int d) {
    return ((d & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0);
}

// 16-byte path: the row's NV chunks through a range-checked descriptor (common.h) of the row's 4 * d bytes, or of none for a
// null operand - straight-line code, no guard per chunk: every load of a wave is in flight before the first wait
template <int NV>
__device__ __forceinline__ void row_load_buf(RowRegs<NV>& r, const float* p, int d, int lane) {
    const m2f_rsrc_t rs = m2f_make_rsrc(p, 4u * (uint32_t)d);
#pragma unroll
    for (int j = 0; j < NV; ++j)
        r.v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * (lane + 64 * j), 0, 0));
}

// 16-byte path, write-through result stores (M2F_WT_ROWS, common.h): the row's NV chunks - and the 8-byte pieces of its bf16 shadow -
// through a descriptor of the row's bytes; chunks behind the row's end are dropped by the range check.  Same values, same bytes as
// row_store / row_store_bf16 (d % 4 == 0 here; the shadow of a 16-byte aligned fp32 row is 8-byte aligned).
template <int NV>
__device__ __forceinline__ void row_store_wt(const RowRegs<NV>& r, float* p, int d, int lane) {
    const m2f_rsrc_t rs = m2f_make_rsrc(p, 4u * (uint32_t)d);
#pragma unroll
    for (int j = 0; j < NV; ++j) m2f_store_b128<true>(rs, 16u * (uint32_t)(lane + 64 * j), r.v[j]);
}
template <int NV>
__device__ __forceinline__ void row_store_bf16_wt(const RowRegs<NV>& r, uint16_t* q, int d, int lane) {
    const m2f_rsrc_t rs = m2f_make_rsrc(q, 2u * (uint32_t)d);
#pragma unroll
    for (int j = 0; j < NV; ++j)
        m2f_store_b64<true>(rs, 8u * (uint32_t)(lane + 64 * j), (uint32_t)m2f_bf16_bits(r.v[j][0]) | ((uint32_t)m2f_bf16_bits(r.v[j][1]) << 16),
                            (uint32_t)m2f_bf16_bits(r.v[j][2]) | ((uint32_t)m2f_bf16_bits(r.v[j][3]) << 16));
}
// one body for both policies: the 16-byte path of a write-through build stores through the descriptor, everything else as before
template <int NV, bool VEC>
__device__ __forceinline__ void ln_store(const RowRegs<NV>& r, float* p, int d, int lane) {
    if constexpr (VEC && M2F_WT_ROWS) row_store_wt(r, p, d, lane);
    else row_store(r, p, d, VEC, lane);
}
template <int NV, bool VEC>
__device__ __forceinline__ void ln_store_bf16(const RowRegs<NV>& r, uint16_t* q, int d, int lane) {
    if constexpr (VEC && M2F_WT_ROWS) {
        if ((reinterpret_cast<uintptr_t>(q) & 7) == 0) { row_store_bf16_wt(r, q, d, lane); return; }      // (wave-uniform)
    }
    row_store_bf16(r, q, d, lane);
}

// the problem a workgroup belongs to: bb[] is ascending (INT_MAX in unused slots), fetched as one 16-byte block, no branches
__device__ __forceinline__ int ln_problem_of(const LnBatch& lb) {
    static_assert(M2F_LN_MAX_PROBLEMS == 4, "the search below reads bb[1..3]");
    const int blk = (int)blockIdx.x;
    return (blk >= lb.bb[1] ? 1 : 0) + (blk >= lb.bb[2] ? 1 : 0) + (blk >= lb.bb[3] ? 1 : 0);
}

// VEC: the launch-uniform 16-byte path (d % 4 == 0, every operand 16-byte aligned) - loads through row_load_buf, the dropout state
// with them; otherwise the general path (any d, any alignment) with guarded element loads.  One body: the arithmetic is stated once.
template <int NV, bool VEC>
__device__ __forceinline__ void ln_fwd_body(const LnBatch& lb, const LnProblem& P, const int pi, const int lane, const int wave) {
    const int d = P.d;
    const int ld = P.ld ? P.ld : d;
    const int blk = (int)blockIdx.x - P.block_begin;
    uint16_t* out16 = m2f_shadow_of(lb.sh, P.out);
    RowRegs<NV> g, be;
    u32x4 rw = {0u, 0u, 0u, 0u};
    uint32_t key = 0;
    if constexpr (VEC) {
        row_load_buf(g, P.gamma, d, lane);
        row_load_buf(be, P.beta, d, lane);
        rw = m2f_rng_words(lb.rng);
    } else {
        row_load(g, P.gamma, d, false, lane);
        row_load(be, P.beta, d, false, lane);
        if (P.drop_site) key = m2f_site_key(lb.rng, P.drop_site);
    }
    const float invd = 1.0f / (float)d;
    for (int rr = 0; rr < LN_ROWS_PER_WAVE; ++rr) {
        const int row = blk * M2F_LN_ROWS_PER_BLOCK + wave * LN_ROWS_PER_WAVE + rr;
        if (row >= lb.T) break;                             // wave-uniform
        RowRegs<NV> x, res;
        if constexpr (VEC) {                                // x and the residual row (no bytes for a null res) with gamma / beta / the state
            row_load_buf(x, P.x + (size_t)row * ld, d, lane);
            row_load_buf(res, P.res ? P.res + (size_t)row * ld : nullptr, d, lane);
            __builtin_amdgcn_sched_barrier(0);              // (the whole batch is issued before anything waits)
        } else {
            row_load(x, P.x + (size_t)row * ld, d, false, lane);
        }
        float mean, rstd;
        if (lb.pre_stats) {                                 // (diagnostic: statistics from memory, no reductions - block-uniform branch)
            mean = P.stats[2 * row]; rstd = P.stats[2 * row + 1];
        } else {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) s += (x.v[j][0] + x.v[j][1]) + (x.v[j][2] + x.v[j][3]);
            mean = m2f_wave_sum(s) * invd;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = 4 * (lane + 64 * j) + e;
                    const float t = (c < d) ? x.v[j][e] - mean : 0.f;
                    q += t * t;
                }
            rstd = 1.0f / sqrtf(m2f_wave_sum(q) * invd + lb.eps);
        }
        if constexpr (VEC) {
            if (rr == 0) {                                  // (x, issued behind the state words, has been waited for)
                m2f_rng_words_arrived(rw);
                if (P.drop_site) key = m2f_site_key_words(rw, P.drop_site);
            }
        } else {
            if (P.res) row_load(res, P.res + (size_t)row * ld, d, false, lane);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y = (x.v[j][e] - mean) * rstd * g.v[j][e] + be.v[j][e];
                if (P.res) y += res.v[j][e];
                if (P.drop_site) {
                    const int c = 4 * (lane + 64 * j) + e;
                    y = m2f_keep(key, (uint32_t)row * (uint32_t)d + (uint32_t)c, lb.drop_thresh) ? y * lb.drop_scale : 0.f;
                }
                x.v[j][e] = y;
            }
        ln_store<NV, VEC>(x, P.out + (size_t)row * ld, d, lane);
        if (out16) ln_store_bf16<NV, VEC>(x, out16 + (size_t)row * ld, d, lane);
        if (lb.out8 && pi == 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = 4 * (lane + 64 * j);
                if (c + 3 < d)
                    *reinterpret_cast<uint32_t*>(lb.out8 + (size_t)row * d + c) =
                        m2f_fp8x4_bits(x.v[j][0] * lb.out8_scale, x.v[j][1] * lb.out8_scale, x.v[j][2] * lb.out8_scale, x.v[j][3] * lb.out8_scale);
            }
        }
        if constexpr (VEC && M2F_WT_ROWS) {                 // the row's statistics: one 8-byte piece (the array is 8-byte aligned per row)
            if (lane == 0) m2f_store_b64<true>(m2f_make_rsrc(P.stats + 2 * (size_t)row, 8), 0, __builtin_bit_cast(uint32_t, mean), __builtin_bit_cast(uint32_t, rstd));
        } else if (lane == 0) { P.stats[2 * row] = mean; P.stats[2 * row + 1] = rstd; }
    }
}

template <int NV>
__global__ __launch_bounds__(256) void m2f_ln_fwd_kernel(const LnBatch lb) {
    static_assert(sizeof(LnBatch) + 64 <= 136 + 512, "m2f_kernarg_warm ranges no longer cover LnBatch + the hidden arguments");
    m2f_kernarg_warm<0, 8, 136>();                  // the descriptor block (552 B + hidden arguments) in one miss
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pi = ln_problem_of(lb);
    const LnProblem P = lb.pr[pi];                  // by value: the problem's fields arrive in a few wide scalar loads
    const int d = P.d;
    const int ld = P.ld ? P.ld : d;
    const bool vec = is_vec(P.x, d) && is_vec(P.out, d) && is_vec(P.gamma, d) && is_vec(P.beta, d) &&
                     (!P.res || is_vec(P.res, d)) && ((ld & 3) == 0);
    if (vec) ln_fwd_body<NV, true>(lb, P, pi, lane, wave);          // launch-uniform
    else ln_fwd_body<NV, false>(lb, P, pi, lane, wave);
}

template <int NV, bool VEC>
__device__ __forceinline__ void ln_bwd_body(const LnBatch& lb, const LnProblem& P, float* red, const int lane, const int wave) {
    const int d = P.d;
    const int ld = P.ld ? P.ld : d;
    const int dpad = (d + 3) & ~3;
    const int blk = (int)blockIdx.x - P.block_begin;
    uint16_t* dx16 = (P.skip & 2) ? nullptr : m2f_shadow_of(lb.sh, P.dx);
    uint16_t* dxm16 = P.dx_masked ? m2f_shadow_of(lb.sh, P.dx_masked) : nullptr;
    const bool dxm32 = P.dx_masked && !((P.skip & 1) && dxm16);
    RowRegs<NV> g, dg, db;
    u32x4 rw = {0u, 0u, 0u, 0u};
    uint32_t key = 0;
    if constexpr (VEC) {
        row_load_buf(g, P.gamma, d, lane);
        rw = m2f_rng_words(lb.rng);
    } else {
        row_load(g, P.gamma, d, false, lane);
        if (P.drop_site2) key = m2f_site_key(lb.rng, P.drop_site2);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) { dg.v[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; db.v[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const float invd = 1.0f / (float)d;
    for (int rr = 0; rr < LN_ROWS_PER_WAVE; ++rr) {
        const int row = blk * M2F_LN_ROWS_PER_BLOCK + wave * LN_ROWS_PER_WAVE + rr;
        if (row >= lb.T) break;
        RowRegs<NV> x, dy, ex;                                  // x, dy, extra and the row's statistics: one batch of loads
        float mean, rstd;
        if constexpr (VEC) {
            row_load_buf(x, P.x + (size_t)row * ld, d, lane);
            row_load_buf(dy, P.dy + (size_t)row * ld, d, lane);
            const m2f_rsrc_t rst = m2f_make_rsrc(P.stats + 2 * (size_t)row, 8);
            const uint32_t st0 = __builtin_amdgcn_raw_buffer_load_b32(rst, 0, 0, 0), st1 = __builtin_amdgcn_raw_buffer_load_b32(rst, 4, 0, 0);
            row_load_buf(ex, P.extra ? P.extra + (size_t)row * ld : nullptr, d, lane);
            __builtin_amdgcn_sched_barrier(0);                  // (left alone, the scheduler moves extra's loads behind the first wait)
            mean = __builtin_bit_cast(float, st0); rstd = __builtin_bit_cast(float, st1);
        } else {
            row_load(x, P.x + (size_t)row * ld, d, false, lane);
            row_load(dy, P.dy + (size_t)row * ld, d, false, lane);
            if (P.extra) row_load(ex, P.extra + (size_t)row * ld, d, false, lane);
            mean = P.stats[2 * row]; rstd = P.stats[2 * row + 1];
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * (lane + 64 * j) + e;
                const float xh = (c < d) ? (x.v[j][e] - mean) * rstd : 0.f;
                const float gy = dy.v[j][e] * g.v[j][e];
                x.v[j][e] = xh;
                s1 += gy;
                s2 += gy * xh;
                dg.v[j][e] += dy.v[j][e] * xh;
                db.v[j][e] += dy.v[j][e];
            }
        const float c1 = m2f_wave_sum(s1) * invd, c2 = m2f_wave_sum(s2) * invd;
        if constexpr (VEC) {
            if (rr == 0) {                                      // (x and dy, issued behind the state words, have been waited for)
                m2f_rng_words_arrived(rw);
                if (P.drop_site2) key = m2f_site_key_words(rw, P.drop_site2);
            }
        }
        RowRegs<NV> msk;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dx = rstd * (dy.v[j][e] * g.v[j][e] - c1 - x.v[j][e] * c2);
                float dm = dx;
                if (P.drop_site2) {
                    const int c = 4 * (lane + 64 * j) + e;
                    dm = m2f_keep(key, (uint32_t)row * (uint32_t)d + (uint32_t)c, lb.drop_thresh) ? dx * lb.drop_scale : 0.f;
                }
                msk.v[j][e] = dm;
                dy.v[j][e] = P.extra ? dx + ex.v[j][e] : dx;
            }
        ln_store<NV, VEC>(dy, P.dx + (size_t)row * ld, d, lane);
        if (dx16) ln_store_bf16<NV, VEC>(dy, dx16 + (size_t)row * ld, d, lane);
        if (dxm32) ln_store<NV, VEC>(msk, P.dx_masked + (size_t)row * ld, d, lane);
        if (dxm16) ln_store_bf16<NV, VEC>(msk, dxm16 + (size_t)row * ld, d, lane);
    }
    // per-block partial dgamma / dbeta: waves -> LDS -> fixed-order sum (deterministic)
    float* mine = red + (size_t)wave * 2 * dpad;
    row_store(dg, mine, dpad, true, lane);
    row_store(db, mine + dpad, dpad, true, lane);
    __syncthreads();
    float* out = P.partial + (size_t)blk * 2 * d;
    const m2f_rsrc_t rpart = m2f_make_rsrc(out, 8u * (uint32_t)d);
    for (int c = threadIdx.x; c < 2 * d; c += 256) {
        const int which = c >= d, cc = which ? c - d : c;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < LN_WAVES; ++w) s += red[(size_t)w * 2 * dpad + which * dpad + cc];
        if constexpr (VEC && M2F_WT_ROWS) m2f_store_b32<true>(rpart, 4u * (uint32_t)c, __builtin_bit_cast(uint32_t, s));
        else out[c] = s;
    }
}

template <int NV>
__global__ __launch_bounds__(256) void m2f_ln_bwd_kernel(const LnBatch lb) {
    static_assert(sizeof(LnBatch) + 64 <= 136 + 512, "m2f_kernarg_warm ranges no longer cover LnBatch + the hidden arguments");
    m2f_kernarg_warm<0, 8, 136>();                  // the descriptor block (552 B + hidden arguments) in one miss
    extern __shared__ __attribute__((aligned(16))) float red[];      // [LN_WAVES][2][dpad]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pi = ln_problem_of(lb);
    const LnProblem P = lb.pr[pi];                  // by value: the problem's fields arrive in a few wide scalar loads
    const int d = P.d;
    const int ld = P.ld ? P.ld : d;
    const bool vec = is_vec(P.x, d) && is_vec(P.dy, d) && is_vec(P.dx, d) && is_vec(P.gamma, d) &&
                     (!P.extra || is_vec(P.extra, d)) && (!P.dx_masked || is_vec(P.dx_masked, d)) && ((ld & 3) == 0);
    if (vec) ln_bwd_body<NV, true>(lb, P, red, lane, wave);         // launch-uniform
    else ln_bwd_body<NV, false>(lb, P, red, lane, wave);
}

// one block = 64 columns of one LayerNorm; its 4 wavefronts each sum a quarter of the row-block partials, then a
// fixed-order LDS combine (deterministic).  Grid (ceil(max_d / 64), items).
// ACC (the accumulate form): dgamma / dbeta = old + the sum, one rounded add of the value the overwrite form stores
template <bool ACC>
__global__ __launch_bounds__(256) void m2f_ln_param_reduce_kernel(const LnReduceBatch rb) {
    __shared__ float part[4][2][64];
    const LnReduceItem& it = rb.it[blockIdx.y];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float sg = 0.f, sb = 0.f;
    if (c < it.d) {
        const int per = (it.nblk + 3) / 4;
        const int b0 = w * per, b1 = b0 + per < it.nblk ? b0 + per : it.nblk;
        // batches of 8 row blocks: 16 independent loads in flight per lane, summed in the fixed order b0, b0+1, ...
        int b = b0;
        for (; b + 8 <= b1; b += 8) {
            float g[8], be[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                g[u] = it.partial[(size_t)(b + u) * 2 * it.d + c];
                be[u] = it.partial[(size_t)(b + u) * 2 * it.d + it.d + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { sg += g[u]; sb += be[u]; }
        }
        for (; b < b1; ++b) {
            sg += it.partial[(size_t)b * 2 * it.d + c];
            sb += it.partial[(size_t)b * 2 * it.d + it.d + c];
        }
    }
    part[w][0][lane] = sg;
    part[w][1][lane] = sb;
    __syncthreads();
    if (w == 0 && c < it.d) {
        const float dg = (part[0][0][lane] + part[1][0][lane]) + (part[2][0][lane] + part[3][0][lane]);
        const float db = (part[0][1][lane] + part[1][1][lane]) + (part[2][1][lane] + part[3][1][lane]);
        if constexpr (ACC) { it.dgamma[c] = it.dgamma[c] + dg; it.dbeta[c] = it.dbeta[c] + db; }
        else { it.dgamma[c] = dg; it.dbeta[c] = db; }
    }
}

// ---- criterion ---------------------------------------------------------------------------------------
// One lane per token row; the row itself and what each criterion adds to it are criterion_row.h's helpers (the ONE definition - the
// reasons for every select and every order of operations are there).  The four kernels stay separate entry points: their register
// budgets differ, and the build's spill gate counts them by name.  An invalid row (label -1 or out of range) is a SELECT of zeros,
// whatever its logits, its teacher row or its twin row hold (NaN, inf).
__global__ __launch_bounds__(256) void m2f_ce_kernel(const CeArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    CeRow r;
    m2f_ce_row_forward(r, a.logits, a.labels, a.class_w, a.label_smoothing, t, a.C);
    a.loss_terms[2 * t] = r.num;
    a.loss_terms[2 * t + 1] = r.valid ? r.wy : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < a.C) a.dlogits[(size_t)t * a.C + c] = m2f_ce_row_grad(r, c, m2f_ce_row_p(r, c));
    }
}

// Distillation criterion (CeArgs::teacher, ::hyper): the plain terms blended with the temperature-scaled KL divergence from a
// teacher's logits.
__global__ __launch_bounds__(256) void m2f_ce_distill_kernel(const CeArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    CeRow r;
    m2f_ce_row_forward(r, a.logits, a.labels, a.class_w, a.label_smoothing, t, a.C);
    CeTeacher k;
    m2f_ce_row_teacher(k, r, a.teacher, t, a.hyper[0], a.hyper[1]);
    float kl = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < a.C) {
            const float d = m2f_ce_teacher_class(k, c, kl);
            const float g = m2f_ce_row_grad(r, c, m2f_ce_row_p(r, c));
            a.dlogits[(size_t)t * a.C + c] = r.valid ? (k.oma * g + k.gd * d) : 0.f;
        }
    }
    a.loss_terms[2 * t] = r.valid ? (k.oma * r.num + k.kd * kl) : 0.f;
    a.loss_terms[2 * t + 1] = r.valid ? r.wy : 0.f;
}

// Focal criterion (CeArgs::gamma; TEACHER: with the distillation blend, the factor scales the hard-label term only)
template <bool TEACHER>
__global__ __launch_bounds__(256) void m2f_ce_focal_kernel(const CeArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    CeRow r;
    m2f_ce_row_forward(r, a.logits, a.labels, a.class_w, a.label_smoothing, t, a.C);
    CeFocal f;
    m2f_ce_row_focal(f, r, a.gamma[0]);
    CeTeacher k;
    if constexpr (TEACHER) m2f_ce_row_teacher(k, r, a.teacher, t, a.hyper[0], a.hyper[1]);
    float kl = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < a.C) {
            const float gf = m2f_ce_focal_grad(f, r, c, m2f_ce_row_grad(r, c, f.p[c]));
            if constexpr (TEACHER) {
                const float d = m2f_ce_teacher_class(k, c, kl);
                a.dlogits[(size_t)t * a.C + c] = r.valid ? (k.oma * gf + k.gd * d) : 0.f;
            } else {
                a.dlogits[(size_t)t * a.C + c] = r.valid ? gf : 0.f;
            }
        }
    }
    if constexpr (TEACHER) a.loss_terms[2 * t] = r.valid ? (k.oma * f.num_f + k.kd * kl) : 0.f;
    else a.loss_terms[2 * t] = r.valid ? f.num_f : 0.f;
    a.loss_terms[2 * t + 1] = r.valid ? r.wy : 0.f;
}

// R-Drop criterion (CeArgs::partner, ::alpha, ::kl_terms): the plain terms plus alpha * w_y times the symmetric KL divergence between
// the row's softmax and its twin's (the same utterance under another dropout mask, row partner[t] of the SAME logits buffer); a row
// reads its twin's logits and writes only its own outputs.  alpha = 0 gives m2f_ce_kernel's bits: x + 0 * finite is exact.
// The twin load is range-checked: an index outside [0, T) means no twin, the lane then re-reads its own row and SELECTS the plain term.
__global__ __launch_bounds__(256) void m2f_ce_rdrop_kernel(const CeArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    const float alpha = a.alpha[0];
    const int tw = a.partner[t];
    const bool has = (tw >= 0) && (tw < a.T);
    CeRow r;
    m2f_ce_row_forward(r, a.logits, a.labels, a.class_w, a.label_smoothing, t, a.C);
    CeTwin k;
    m2f_ce_row_twin(k, r, a.logits, has ? tw : t, has);
    const float ak = alpha * r.wy;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < a.C) {
            const float g = m2f_ce_row_grad(r, c, m2f_ce_row_p(r, c));
            a.dlogits[(size_t)t * a.C + c] = r.valid ? (g + ak * m2f_ce_twin_grad(k, c)) : 0.f;
        }
    }
    a.loss_terms[2 * t] = r.valid ? (r.num + alpha * k.ws) : 0.f;
    a.loss_terms[2 * t + 1] = r.valid ? r.wy : 0.f;
    a.kl_terms[t] = k.ws;
}

// The KL share of the R-Drop numerator on its own: loss_out[3] = sum of kl_terms (w_y * s per row, without alpha).  ACC: added, as
// the finalize launch adds den and num.
template <bool ACC>
__global__ __launch_bounds__(256) void m2f_rdrop_kl_reduce_kernel(const float* __restrict__ kl_terms, int T, float* __restrict__ loss_out) {
    float kl[1];
    m2f_block_sum_terms<1>(kl_terms, T, kl);
    if (threadIdx.x == 0) {
        if constexpr (ACC) loss_out[3] = loss_out[3] + kl[0];
        else loss_out[3] = kl[0];
    }
}

// ACC (the accumulate form): den and num are added to loss_out[1], loss_out[2] (a group of micro-batches); loss_out[0] stays this batch's
template <bool ACC>
__global__ __launch_bounds__(256) void m2f_loss_finalize_kernel(const float* __restrict__ terms, int T, int C,
                                                                float* __restrict__ dlogits, float* __restrict__ loss_out,
                                                                int normalise) {
    float s[2];
    m2f_block_sum_terms<2>(terms, T, s);
    const float num = s[0], den = s[1];
    if constexpr (ACC) {
        if (threadIdx.x == 0) { loss_out[0] = num / den; loss_out[1] = loss_out[1] + den; loss_out[2] = loss_out[2] + num; }
    } else {
        if (threadIdx.x == 0) { loss_out[0] = num / den; loss_out[1] = den; loss_out[2] = num; }
    }
    if (normalise) {
        const float inv = 1.0f / den;
        for (int e = threadIdx.x; e < T * C; e += 256) dlogits[e] *= inv;
    }
}

// (blockIdx.y = 1: the second buffer of the launch - the two modalities' post-projection gradients share one launch)
__global__ __launch_bounds__(256) void m2f_dropout_inplace_kernel(float* __restrict__ x0, float* __restrict__ x1, int T, int d, int ld,
                                                                  uint32_t site0, uint32_t site1, const uint32_t* __restrict__ rng,
                                                                  uint32_t thresh, float scale, ShadowMap sh) {
    float* __restrict__ x = blockIdx.y ? x1 : x0;
    const uint32_t key = m2f_site_key(rng, blockIdx.y ? site1 : site0);
    const size_t n = (size_t)T * d;
    uint16_t* x16 = m2f_shadow_of(sh, x);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / d), c = (int)(e - (size_t)r * d);
        float* p = x + (size_t)r * ld + c;
        const float v = m2f_keep(key, (uint32_t)e, thresh) ? *p * scale : 0.f;
        *p = v;
        if (x16) x16[(size_t)r * ld + c] = m2f_bf16_bits(v);
    }
}

// fp32 -> bf16 copies of 2-D blocks (parameter matrices into their padded shadows, input staging buffers)
__global__ __launch_bounds__(256) void m2f_cast_kernel(const CastBatch cb) {
    const CastItem& it = cb.it[blockIdx.y];
    const size_t n4 = (size_t)it.rows * ((it.cols + 3) >> 2);
    const int c4n = (it.cols + 3) >> 2;
    const bool vec = ((it.cols & 3) == 0) && ((it.lds & 3) == 0) && ((it.ldd & 3) == 0) &&
                     ((reinterpret_cast<uintptr_t>(it.src) & 15) == 0) && ((reinterpret_cast<uintptr_t>(it.dst) & 7) == 0);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / c4n), c = 4 * (int)(i - (size_t)r * c4n);
        const float* s = it.src + (size_t)r * it.lds + c;
        uint16_t* q = it.dst + (size_t)r * it.ldd + c;
        if (vec) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(s);
            uint2 w;
            w.x = (uint32_t)m2f_bf16_bits(x[0]) | ((uint32_t)m2f_bf16_bits(x[1]) << 16);
            w.y = (uint32_t)m2f_bf16_bits(x[2]) | ((uint32_t)m2f_bf16_bits(x[3]) << 16);
            *reinterpret_cast<uint2*>(q) = w;
        } else {
            for (int e = 0; e < 4; ++e) if (c + e < it.cols) q[e] = m2f_bf16_bits(s[e]);
        }
    }
}

// one wavefront per token slot: two row copies (16-byte pieces when aligned) + label / mask
__global__ __launch_bounds__(256) void m2f_gather_kernel(const GatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T) return;
    const int row = a.rows[t];
    const bool pad = row < 0;
    for (int which = 0; which < 2; ++which) {
        const float* tab = which ? a.audio_table : a.text_table;
        float* out = which ? a.audio_out : a.text_out;
        const int d = which ? a.d_audio : a.d_text, ld = which ? a.ld_audio : a.ld_text;
        if (!tab || !out) continue;
        const float* src = tab + (size_t)(pad ? 0 : row) * d;
        float* dst = out + (size_t)t * ld;
        const bool vec = ((d & 3) == 0) && ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(tab) & 15) == 0) &&
                         ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
        if (vec) {
            for (int c = 4 * lane; c < d; c += 256) {
                f32x4 x = *reinterpret_cast<const f32x4*>(src + c);
                if (pad) x = (f32x4){0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(dst + c) = x;
            }
        } else {
            for (int c = lane; c < d; c += 64) dst[c] = pad ? 0.f : src[c];
        }
    }
    if (lane == 0) {
        if (a.key_pad) a.key_pad[t] = pad ? 1 : 0;
        if (a.labels) a.labels[t] = (pad || !a.label_table) ? -1 : a.label_table[row];
    }
}

__global__ void m2f_rng_advance_kernel(uint32_t* rng) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const uint32_t lo = rng[2] + 1u;
        rng[2] = lo;
        if (lo == 0u) rng[3] += 1u;
    }
}

template <bool BWD>
hipError_t ln_launch(LnBatch& lb, hipStream_t stream) {
    if (lb.count <= 0 || lb.count > M2F_LN_MAX_PROBLEMS || lb.T <= 0) return hipErrorInvalidValue;
    int blocks = 0, maxd = 0;
    for (int i = 0; i < M2F_LN_MAX_PROBLEMS; ++i) lb.bb[i] = 0x7fffffff;
    for (int i = 0; i < lb.count; ++i) {
        LnProblem& p = lb.pr[i];
        if (p.d < 1 || p.d > 256 * LN_MAXV_LIMIT) return hipErrorInvalidValue;
        if ((p.drop_site || p.drop_site2) && !lb.rng) return hipErrorInvalidValue;
        p.block_begin = blocks;
        lb.bb[i] = blocks;
        blocks += m2f_ln_row_blocks(lb.T);
        if (p.d > maxd) maxd = p.d;
    }
    const size_t lds = BWD ? (size_t)LN_WAVES * 2 * ((maxd + 3) & ~3) * sizeof(float) : 0;
    const int nv = m2f_cdiv(maxd, 256);
#define M2F_LN_CASE(N)                                                                                      \
    if (nv <= N) {                                                                                          \
        if (BWD) hipLaunchKernelGGL(m2f_ln_bwd_kernel<N>, dim3(blocks), dim3(256), lds, stream, lb);        \
        else hipLaunchKernelGGL(m2f_ln_fwd_kernel<N>, dim3(blocks), dim3(256), 0, stream, lb);              \
        return hipGetLastError();                                                                           \
    }
    M2F_LN_CASE(1)
    M2F_LN_CASE(2)
    M2F_LN_CASE(3)
    M2F_LN_CASE(4)
    M2F_LN_CASE(8)
#undef M2F_LN_CASE
    return hipGetLastError();
}

}  // namespace

hipError_t m2f_launch_ln_fwd(LnBatch& lb, hipStream_t stream) { return ln_launch<false>(lb, stream); }
hipError_t m2f_launch_ln_bwd(LnBatch& lb, hipStream_t stream) { return ln_launch<true>(lb, stream); }

hipError_t m2f_launch_ln_param_reduce(const LnReduceBatch& rb, hipStream_t stream, int accumulate) {
    if (rb.count <= 0) return hipSuccess;
    if (rb.count > M2F_LNRED_MAX_ITEMS) return hipErrorInvalidValue;
    int maxd = 0;
    for (int i = 0; i < rb.count; ++i) if (rb.it[i].d > maxd) maxd = rb.it[i].d;
    if (accumulate) hipLaunchKernelGGL(m2f_ln_param_reduce_kernel<true>, dim3(m2f_cdiv(maxd, 64), rb.count), dim3(256), 0, stream, rb);
    else hipLaunchKernelGGL(m2f_ln_param_reduce_kernel<false>, dim3(m2f_cdiv(maxd, 64), rb.count), dim3(256), 0, stream, rb);
    return hipGetLastError();
}

// The ONE criterion launch: the kernel follows from which optional pointers are set (ops.h, CeArgs)
hipError_t m2f_launch_ce(const CeArgs& a, hipStream_t stream) {
    if (a.C < 1 || a.C > 16 || a.T < 1) return hipErrorInvalidValue;
    if (a.partner ? (a.teacher || a.gamma || !a.alpha || !a.kl_terms) : (a.teacher && !a.hyper)) return hipErrorInvalidValue;
    const dim3 grid(m2f_cdiv(a.T, 256)), block(256);
    if (a.partner) hipLaunchKernelGGL(m2f_ce_rdrop_kernel, grid, block, 0, stream, a);
    else if (a.gamma && a.teacher) hipLaunchKernelGGL(m2f_ce_focal_kernel<true>, grid, block, 0, stream, a);
    else if (a.gamma) hipLaunchKernelGGL(m2f_ce_focal_kernel<false>, grid, block, 0, stream, a);
    else if (a.teacher) hipLaunchKernelGGL(m2f_ce_distill_kernel, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(m2f_ce_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t m2f_launch_rdrop_kl_reduce(const float* kl_terms, int T, float* loss_out, hipStream_t stream, int accumulate) {
    if (!kl_terms || !loss_out || T < 1) return hipErrorInvalidValue;
    if (accumulate) hipLaunchKernelGGL(m2f_rdrop_kl_reduce_kernel<true>, dim3(1), dim3(256), 0, stream, kl_terms, T, loss_out);
    else hipLaunchKernelGGL(m2f_rdrop_kl_reduce_kernel<false>, dim3(1), dim3(256), 0, stream, kl_terms, T, loss_out);
    return hipGetLastError();
}

hipError_t m2f_launch_loss_finalize(const float* loss_terms, int T, int C, float* dlogits, float* loss_out,
                                    int normalise, hipStream_t stream, int accumulate) {
    if (accumulate) hipLaunchKernelGGL(m2f_loss_finalize_kernel<true>, dim3(1), dim3(256), 0, stream, loss_terms, T, C, dlogits, loss_out, normalise);
    else hipLaunchKernelGGL(m2f_loss_finalize_kernel<false>, dim3(1), dim3(256), 0, stream, loss_terms, T, C, dlogits, loss_out, normalise);
    return hipGetLastError();
}

hipError_t m2f_launch_dropout_inplace2(float* x, float* x2, int T, int d, int ld, uint32_t site, uint32_t site2, const uint32_t* rng,
                                       uint32_t thresh, float scale, ShadowMap sh, hipStream_t stream) {
    const size_t n = (size_t)T * d;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(m2f_dropout_inplace_kernel, dim3(blocks, x2 ? 2 : 1), dim3(256), 0, stream, x, x2, T, d, ld, site, site2, rng, thresh,
                       scale, sh);
    return hipGetLastError();
}
hipError_t m2f_launch_dropout_inplace(float* x, int T, int d, int ld, uint32_t site, const uint32_t* rng,
                                      uint32_t thresh, float scale, ShadowMap sh, hipStream_t stream) {
    return m2f_launch_dropout_inplace2(x, nullptr, T, d, ld, site, 0u, rng, thresh, scale, sh, stream);
}

// ---- 64x64 transposing tile: src fp32 [rows][ld] -> bf16 dst [rows][ldd] (optional) and bf16 dst_t [cols][ldt] ------------
// 16-byte loads (4 floats of a row per lane), 8-byte stores of the plain copy, and - through an LDS tile - 16-byte stores
// of the transposed copy (8 consecutive source rows of one column per lane), so all three streams move full 128-byte
// lines.  Source elements outside [rows) x [cols) read as zero, which also writes the zero pads of dst_t up to ldt.
// cs[4] accumulates this thread's four column sums of the (pre-relu) source.
template <bool PLAIN>
__device__ __forceinline__ void m2f_tile64(const float* __restrict__ src, int ld, int rows, int cols, int r0, int c0,
                                           uint16_t* __restrict__ dst, int ldd, uint16_t* __restrict__ dst_t, int ldt,
                                           bool relu, bool vec, float (&cs)[4], float (*tile)[65]) {
    const int tid = threadIdx.x;
    const int lr = tid >> 4, c = 4 * (tid & 15);
    const int gc = c0 + c;
    f32x4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                       // unconditional clamped loads, select afterwards
        const int gr = r0 + lr + 16 * i;
        const int grc = gr < rows ? gr : rows - 1;
        if (vec && gc + 3 < cols) {
            x[i] = *reinterpret_cast<const f32x4*>(src + (size_t)grc * ld + gc);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[i][e] = src[(size_t)grc * ld + (gc + e < cols ? gc + e : cols - 1)];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = lr + 16 * i, gr = r0 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = (gr < rows && gc + e < cols) ? x[i][e] : 0.f;
            cs[e] += v;
            if (relu) v = fmaxf(v, 0.f);
            x[i][e] = v;
            tile[r][c + e] = v;
        }
        if (PLAIN && gr < rows) {
            uint16_t* q = dst + (size_t)gr * ldd + gc;
            if (vec && gc + 3 < cols && (ldd & 3) == 0) {
                uint2 w;
                w.x = (uint32_t)m2f_bf16_bits(x[i][0]) | ((uint32_t)m2f_bf16_bits(x[i][1]) << 16);
                w.y = (uint32_t)m2f_bf16_bits(x[i][2]) | ((uint32_t)m2f_bf16_bits(x[i][3]) << 16);
                *reinterpret_cast<uint2*>(q) = w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (gc + e < cols) q[e] = m2f_bf16_bits(x[i][e]);
            }
        }
    }
    __syncthreads();
    if (dst_t) {                                                        // block-uniform
        const int r8 = tid & 7;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cc = (tid >> 3) + 32 * j;                         // source column = row of dst_t
            const int gcol = c0 + cc, gr0 = r0 + 8 * r8;                // 8 consecutive source rows = 8 consecutive dst_t columns
            if (gcol < cols && gr0 < ldt) {
                uint16_t h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) h[k] = m2f_bf16_bits(tile[8 * r8 + k][cc]);
                uint16_t* q = dst_t + (size_t)gcol * ldt + gr0;
                if ((ldt & 7) == 0 && ((reinterpret_cast<uintptr_t>(dst_t) & 15) == 0)) {
                    uint4 w;
                    w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
                    w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
                    *reinterpret_cast<uint4*>(q) = w;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) if (gr0 + k < ldt) q[k] = h[k];
                }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool m2f_tile_vec_ok(const float* src, int ld) {
    return ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(src) & 15) == 0);
}

// parameter matrix -> padded bf16 shadow + transposed padded bf16 shadow
__global__ __launch_bounds__(256) void m2f_cast_t_kernel(const CastBatch cb) {
    __shared__ float tile[64][65];
    const CastItem& it = cb.it[blockIdx.y];
    const int tiles_c = (it.cols + 63) >> 6, tiles_r = (it.rows + 63) >> 6;
    const bool vec = m2f_tile_vec_ok(it.src, it.lds);
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = blockIdx.x; t < tiles_c * tiles_r; t += gridDim.x) {
        const int r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
        m2f_tile64<true>(it.src, it.lds, it.rows, it.cols, r0, c0, it.dst, it.ldd, it.dst_t, it.ldd_t, false, vec, cs, tile);
    }
}

hipError_t m2f_launch_cast(const CastBatch& cb, hipStream_t stream) {
    if (cb.count <= 0) return hipSuccess;
    if (cb.count > M2F_CAST_MAX_ITEMS) return hipErrorInvalidValue;
    bool transposed = true;
    for (int i = 0; i < cb.count; ++i) transposed = transposed && cb.it[i].dst_t != nullptr;
    if (transposed) {
        size_t mt = 0;
        for (int i = 0; i < cb.count; ++i) mt = std::max(mt, (size_t)((cb.it[i].rows + 63) / 64) * ((cb.it[i].cols + 63) / 64));
        const int bx = (int)std::min<size_t>(std::max<size_t>(mt, 1), 96);
        hipLaunchKernelGGL(m2f_cast_t_kernel, dim3(bx, cb.count), dim3(256), 0, stream, cb);
        return hipGetLastError();
    }
    size_t mx = 0;
    for (int i = 0; i < cb.count; ++i) mx = std::max(mx, (size_t)cb.it[i].rows * ((cb.it[i].cols + 3) / 4));
    int bx = (int)std::min<size_t>((mx + 255) / 256, 512);
    if (bx < 1) bx = 1;
    hipLaunchKernelGGL(m2f_cast_kernel, dim3(bx, cb.count), dim3(256), 0, stream, cb);
    return hipGetLastError();
}

// RoBERTa embeddings (transformers RobertaEmbeddings.forward, used by the reference at
// src/feature_extractors/text/model.py:16,19): LayerNorm(word[ids] + position[pos_ids] + token_type[0]), one wavefront per
// token, d <= 2048 (d % 4 == 0), values in registers.
__global__ __launch_bounds__(256) void m2f_embed_ln_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ pos_ids,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ type0, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                           int ld, int T, int d, ShadowMap sh) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const float* w = word + (size_t)ids[t] * d;
    const float* p = pos + (size_t)pos_ids[t] * d;
    f32x4 x[8];
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = 4 * (lane + 64 * j);
        if (c < d) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(w + c), b = *reinterpret_cast<const f32x4*>(p + c);
            const f32x4 ty = *reinterpret_cast<const f32x4*>(type0 + c);
            x[j] = a + b + ty;
            s1 += (x[j][0] + x[j][1]) + (x[j][2] + x[j][3]);
        } else {
            x[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    const float mean = m2f_wave_sum(s1) / (float)d;
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = 4 * (lane + 64 * j);
        if (c < d) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float dv = x[j][e] - mean; s2 += dv * dv; }
        }
    }
    const float rstd = rsqrtf(m2f_wave_sum(s2) / (float)d + eps);
    float* o = out + (size_t)t * ld;
    uint16_t* o16 = m2f_shadow_of(sh, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = 4 * (lane + 64 * j);
        if (c < d) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c), be = *reinterpret_cast<const f32x4*>(beta + c);
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (x[j][e] - mean) * rstd * g[e] + be[e];
            *reinterpret_cast<f32x4*>(o + c) = y;
            if (o16) {
                uint2 h;
                h.x = (uint32_t)m2f_bf16_bits(y[0]) | ((uint32_t)m2f_bf16_bits(y[1]) << 16);
                h.y = (uint32_t)m2f_bf16_bits(y[2]) | ((uint32_t)m2f_bf16_bits(y[3]) << 16);
                *reinterpret_cast<uint2*>(o16 + c) = h;
            }
        }
    }
}

hipError_t m2f_launch_embed_ln(const int64_t* ids, const int64_t* pos_ids, const float* word, const float* pos, const float* type0,
                               const float* gamma, const float* beta, float eps, float* out, int ld, int T, int d, ShadowMap sh,
                               hipStream_t stream) {
    if (T < 1 || d < 4 || d > 2048 || (d & 3) || (ld & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_embed_ln_kernel, dim3(m2f_cdiv(T, 4)), dim3(256), 0, stream, ids, pos_ids, word, pos, type0, gamma, beta,
                       eps, out, ld, T, d, sh);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void m2f_quant_fp8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t n4, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(src)[i];
        reinterpret_cast<uint32_t*>(dst)[i] = m2f_fp8x4_bits(x[0] * scale, x[1] * scale, x[2] * scale, x[3] * scale);
    }
}

hipError_t m2f_launch_quant_fp8(const float* src, uint8_t* dst, int64_t n, float scale, hipStream_t stream) {
    if (n <= 0 || (n & 3) || (reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 3)) return hipErrorInvalidValue;
    const int64_t n4 = n >> 2;
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(m2f_quant_fp8_kernel, dim3(blocks), dim3(256), 0, stream, src, dst, n4, scale);
    return hipGetLastError();
}

hipError_t m2f_launch_gather(const GatherArgs& a, hipStream_t stream) {
    if (a.T < 1 || !a.rows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_gather_kernel, dim3(m2f_cdiv(a.T, 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t m2f_launch_rng_advance(uint32_t* rng, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_rng_advance_kernel, dim3(1), dim3(64), 0, stream, rng);
    return hipGetLastError();
}

// fp32 -> bf16 of the flat-buffer ranges of `items` (whole tensors incl. their pads: rows > 0 -> rows x cols elements, else `cols`): the
// gradients the weight-gradient table launch did NOT write as bf16 itself (biases, LayerNorm, the matrices outside the table) when the
// step leaves its gradients in a bf16 buffer (m2f_plan_grad_bf16); tiles of 4,096 elements, tile -> item by bisection
__global__ __launch_bounds__(256) void m2f_cast_items_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, const AdamItem* __restrict__ items,
                                                            const int* __restrict__ tile_begin, int n_items, int total_tiles) {
    __shared__ int tb[M2F_ADAM_MAX_ITEMS + 1];
    walk_prefix(tb, tile_begin, n_items);
    for (int t = blockIdx.x; t < total_tiles; t += gridDim.x) {
        const WalkTile wt = walk_tile(tb, items, n_items, t);
        const AdamItem& it = wt.it;
        const long long n = it.rows > 0 ? (long long)it.rows * it.cols : (long long)it.cols;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long idx = walk_run_index(wt.tl, q);
            if (idx + 3 < n) {
                *reinterpret_cast<u32x2*>(dst + it.off + idx) = param_bf16x4(*reinterpret_cast<const f32x4*>(src + it.off + idx));
            } else {
                for (int e = 0; e < 4; ++e) if (idx + e < n) dst[it.off + idx + e] = m2f_bf16_bits(src[it.off + idx + e]);
            }
        }
    }
}
hipError_t m2f_launch_cast_items(const float* src, uint16_t* dst, const AdamItem* items, const int* tile_begin, int n_items, int total_tiles, hipStream_t stream) {
    if (n_items < 1 || n_items > M2F_ADAM_MAX_ITEMS || total_tiles < 1 || !items || !tile_begin || !src || !dst) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_cast_items_kernel, dim3(total_tiles < 2048 ? total_tiles : 2048), dim3(256), 0, stream, src, dst, items, tile_begin, n_items, total_tiles);
    return hipGetLastError();
}
