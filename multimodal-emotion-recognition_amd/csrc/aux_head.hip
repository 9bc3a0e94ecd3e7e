// Auxiliary label head: a second linear classifier over the rows of a feature matrix, scored against its own labels, forward and
// backward, exact fp32 on gfx950 whatever the plan's precision.
//
// Definition (AuxHeadArgs, ops.h).  h_i = row i of feat (width D, row stride ld), params = [W (A x D, row-major) | b (A)], 2 <= A <= 16,
// s_i the auxiliary label, y_i the primary (emotion) label with its class weight w_y (1 without class weights).  For every row:
//   u_i   = W h_i + b                                                          (aux_logits, every row)
//   a_i   = label-smoothed cross entropy of u_i against s_i (eps_a, no class weights of its own): criterion_row.h's row, not a copy
//   row_term[i] = w_{y_i} a_i          g[i, c] = w_{y_i} d a_i / d u_ic          both SELECTED to 0 unless 0 <= y_i < C and 0 <= s_i < A
// and, from g (which may also be an upstream gradient: the autograd surface of the head calls the last three with its own g):
//   dh[i, :] (+)= gate_i * scale * lambda * sum_c g[i, c] W[c, :]               gate_i = (h[i, :] > 0 ? gate_scale : 0), or 1 without h
//   dW = scale * lambda * g^T h,  db = scale * lambda * sum_i g[i, :]           a term with g[i, c] == 0 is SELECTED to 0, whatever h holds
//
// The shapes are skinny (A <= 16): the work is the two reads of h and one pass over dh, so nothing here is an MFMA.  Launches:
//   rows    one workgroup per 8 rows, a wave per row in turn: W | b staged into LDS once per workgroup (row-major, rows padded to a
//           multiple of 4 floats: lane l reads the 16 bytes behind column 4 l of a row, consecutive lanes consecutive slots - no bank
//           is asked twice); a row's 16-byte loads of h issued together, the NEXT row's in flight while this one is summed; A
//           lane-strided partial sums, one xor-shuffle tree each; then the row is scored by every lane alike, lane 0 stores
//   tail    one workgroup: the row terms summed in the finalize launch's order into the tail's fourth float, and the scale that
//           launch applies to dlogits (1 / den, the same bits; 1 without normalise)
//   join    one workgroup per 8 rows, W in LDS as above, the sum over c in registers in class order
//   wpart   one workgroup per (64 rows, 256 columns): a wave owns 16 rows, a lane 4 columns, rows in order (four rows' loads issued
//           together) -> part[row block of 16]
//   wred    one thread per element of [W | b]: the partials summed in block order, scaled by scale * lambda, OVERWRITING the gradient
// The grids follow from N (and D) alone, no atomics, every sum has one order: two runs give the same bits.
// Eight rows per workgroup, not more: the shapes are latency-bound, so the rows are spread over many workgroups (T = 1,024: 128) with
// two rows per wave, both in flight, and W | b (at most 64 KB) is re-staged per workgroup from L2.
#include "common.h"
#include "ops.h"
#include "criterion_row.h"

namespace {

constexpr int AH_ROWS = 8;       // rows per workgroup of the rows and join kernels: two per wave, both in flight (T = 1,024: 128 workgroups)
constexpr int AH_WROWS = 16;     // rows per wave of the parameter-gradient partials: one partial block
constexpr int AH_MAXD = 1024;    // W | b in LDS: 16 x 1,024 floats + 16

__device__ __forceinline__ int ah_dp(int D) { return (D + 3) & ~3; }

// [W | b] -> LDS: rows padded with zeros to Dp floats, the bias behind them
__device__ __forceinline__ void ah_stage(float* __restrict__ Ws, const float* __restrict__ params, int A, int D, int Dp) {
    for (int e = threadIdx.x; e < A * Dp; e += blockDim.x) {
        const int c = e / Dp, k = e - c * Dp;
        Ws[e] = k < D ? params[(size_t)c * D + k] : 0.f;
    }
    for (int c = threadIdx.x; c < A; c += blockDim.x) Ws[A * Dp + c] = params[(size_t)A * D + c];
    __syncthreads();
}

// the 16-byte pieces of row t a lane owns (columns 4 (lane + 64 j)), columns past D SELECTED to 0; rows are 16-byte aligned (ld % 4 == 0)
template <int NJ>
__device__ __forceinline__ void ah_load_row(f32x4 (&v)[NJ], const float* __restrict__ feat, int ld, int D, int t, int lane) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 4 * (lane + 64 * j);
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < D) v[j] = *reinterpret_cast<const f32x4*>(feat + (size_t)t * ld + k);      // (k + 3 < ld: ld >= D rounded up to 4)
    }
}

template <int NJ>
__global__ __launch_bounds__(256) void m2f_aux_rows_kernel(const float* __restrict__ feat, int N, int D, int ld,
                                                           const float* __restrict__ params, int A, const int64_t* __restrict__ labels, int C,
                                                           const float* __restrict__ class_w, const int64_t* __restrict__ aux_labels,
                                                           const float* __restrict__ hyper, float* __restrict__ aux_logits, int ldu,
                                                           float* __restrict__ g, float* __restrict__ row_term, float* __restrict__ loss_terms) {
    extern __shared__ __attribute__((aligned(16))) float Ws[];
    const int Dp = ah_dp(D), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    ah_stage(Ws, params, A, D, Dp);
    const float lambda = hyper ? hyper[0] : 0.f, eps = hyper ? hyper[1] : 0.f;      // (hyper, the labels, g and row_term null: the logits alone)
    const int t0 = blockIdx.x * AH_ROWS, t1 = min(t0 + AH_ROWS, N);
    f32x4 cur[NJ], nxt[NJ];
    if (t0 + wv < t1) ah_load_row<NJ>(cur, feat, ld, D, t0 + wv, lane);
    for (int t = t0 + wv; t < t1; t += 4) {
        if (t + 4 < t1) ah_load_row<NJ>(nxt, feat, ld, D, t + 4, lane);
        float u[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            float acc = 0.f;
            if (c < A) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int k = 4 * (lane + 64 * j);
                    if (k < Dp) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(Ws + c * Dp + k);
                        const f32x4 h = cur[j];
                        // (the row's columns past D were selected to 0 where the vector was loaded whole; a vector that straddles D holds
                        // whatever the pad columns hold: select again by column)
                        acc = fmaf(k + 0 < D ? h[0] : 0.f, w[0], acc);
                        acc = fmaf(k + 1 < D ? h[1] : 0.f, w[1], acc);
                        acc = fmaf(k + 2 < D ? h[2] : 0.f, w[2], acc);
                        acc = fmaf(k + 3 < D ? h[3] : 0.f, w[3], acc);
                    }
                }
                acc = m2f_wave_sum(acc) + Ws[A * Dp + c];
            }
            u[c] = acc;
        }
        // the row, by criterion_row.h: its "logits" are u, its label the auxiliary one, no class weights, smoothing eps_a
        if (aux_labels) {
            CeRow r;
            m2f_ce_row_forward(r, u, aux_labels + t, nullptr, eps, 0, A);
            const int64_t y = labels[t];
            const bool live = (y >= 0) && (y < C) && r.valid;
            const float wy = live ? (class_w ? class_w[y] : 1.f) : 0.f;
            if (lane == 0) {
                const float term = live ? wy * r.num : 0.f;
                row_term[t] = term;
                if (loss_terms) loss_terms[2 * (size_t)t] = loss_terms[2 * (size_t)t] + lambda * term;
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < A) g[(size_t)t * 16 + c] = live ? wy * m2f_ce_row_grad(r, c, m2f_ce_row_p(r, c)) : 0.f;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < A) aux_logits[(size_t)t * ldu + c] = u[c];
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) cur[j] = nxt[j];
    }
}

// loss_out[3] = (ACC: +=) sum of the row terms in the finalize launch's order; scale[0] = what that launch multiplies dlogits by
template <bool ACC>
__global__ __launch_bounds__(256) void m2f_aux_tail_kernel(const float* __restrict__ row_term, const float* __restrict__ loss_terms, int T,
                                                           float* __restrict__ loss_out, float* __restrict__ scale, int normalise) {
    float r1[1], s[2];
    m2f_block_sum_terms<1>(row_term, T, r1);
    m2f_block_sum_terms<2>(loss_terms, T, s);
    if (threadIdx.x == 0) {
        if constexpr (ACC) loss_out[3] = loss_out[3] + r1[0];
        else loss_out[3] = r1[0];
        scale[0] = normalise ? (s[1] > 0.f ? 1.0f / s[1] : 0.f) : 1.f;
    }
}

// dh[t, :] = (ADD: dh[t, :] +) gate * (scale * lambda) * sum_c g[t, c] W[c, :], the bf16 shadow of dh rewritten when it has one
template <int NJ>
__global__ __launch_bounds__(256) void m2f_aux_join_kernel(float* __restrict__ dh, int ldd, const float* __restrict__ h, int ld,
                                                           const float* __restrict__ g, int ldg, const float* __restrict__ params, int A, int N, int D,
                                                           const float* __restrict__ scale, const float* __restrict__ hyper, float gate_scale,
                                                           int add, int write16, ShadowMap sh) {
    extern __shared__ __attribute__((aligned(16))) float Ws[];
    const int Dp = ah_dp(D), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    ah_stage(Ws, params, A, D, Dp);
    const float f = (scale ? scale[0] : 1.f) * (hyper ? hyper[0] : 1.f);
    uint16_t* dh16 = write16 ? m2f_shadow_of(sh, dh) : nullptr;
    const int t0 = blockIdx.x * AH_ROWS, t1 = min(t0 + AH_ROWS, N);
    for (int t = t0 + wv; t < t1; t += 4) {
        float gr[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) gr[c] = c < A ? g[(size_t)t * ldg + c] : 0.f;
        f32x4 old[NJ], hv[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {          // (every load of the row first, then the sums)
            const int k = 4 * (lane + 64 * j);
            old[j] = hv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < D) {
                if (add) old[j] = *reinterpret_cast<const f32x4*>(dh + (size_t)t * ldd + k);
                if (h) hv[j] = *reinterpret_cast<const f32x4*>(h + (size_t)t * ld + k);
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = 4 * (lane + 64 * j);
            if (k < D) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < A) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(Ws + c * Dp + k);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = fmaf(gr[c], w[e], acc[e]);
                    }
                const size_t o = (size_t)t * ldd + k;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gate = h ? (hv[j][e] > 0.f ? gate_scale : 0.f) : 1.f;
                    const float v = old[j][e] + gate * (f * acc[e]);
                    if (k + e < D) {            // (the pad columns behind D keep what they hold)
                        dh[o + e] = v;
                        if (dh16) dh16[o + e] = m2f_bf16_bits(v);
                    }
                }
            }
        }
    }
}

// part[blk] = [dW (A x D) | db (A)] of the 16 rows blk * 16 .. + 15, rows in order; blk = 4 * blockIdx.x + wave, columns 256 * blockIdx.y ..
__global__ __launch_bounds__(256) void m2f_aux_wpart_kernel(const float* __restrict__ h, int ld, const float* __restrict__ g, int ldg, int A, int N, int D,
                                                            float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int blk = blockIdx.x * 4 + wv, t0 = blk * AH_WROWS, t1 = min(t0 + AH_WROWS, N);
    if (t0 >= N) return;
    const int k = 256 * blockIdx.y + 4 * lane;
    float* out = part + (size_t)blk * ((size_t)A * D + A);
    f32x4 acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float db = 0.f;
    for (int tb = t0; tb < t1; tb += 4) {
        f32x4 hv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {           // (four rows' loads together, then their sums in row order)
            hv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < D && tb + i < t1) hv[i] = *reinterpret_cast<const f32x4*>(h + (size_t)(tb + i) * ld + k);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = tb + i;
            if (t < t1) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < A) {
                        const float gc = g[(size_t)t * ldg + c];
                        // a SELECT, not a product with 0: an ignored row's h may hold anything (NaN, inf)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[c][e] = gc != 0.f ? fmaf(gc, hv[i][e], acc[c][e]) : acc[c][e];
                    }
                if (blockIdx.y == 0 && lane < A) db += g[(size_t)t * ldg + lane];
            }
        }
    }
    if (k < D) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < A) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < D) out[(size_t)c * D + k + e] = acc[c][e];
            }
    }
    if (blockIdx.y == 0 && lane < A) out[(size_t)A * D + lane] = db;
}

// grad[e] = (scale * lambda) * sum over the partial blocks, in block order
__global__ __launch_bounds__(256) void m2f_aux_wred_kernel(const float* __restrict__ part, int nblk, int n, const float* __restrict__ scale,
                                                           const float* __restrict__ hyper, float* __restrict__ grad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float f = (scale ? scale[0] : 1.f) * (hyper ? hyper[0] : 1.f);
    float s = 0.f;
    for (int b0 = 0; b0 < nblk; b0 += 8) {      // (eight partials' loads together, added in block order)
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = b0 + i < nblk ? part[(size_t)(b0 + i) * n + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (b0 + i < nblk) s += v[i];
    }
    grad[e] = f * s;
}

inline size_t ah_lds_bytes(int A, int D) { return ((size_t)A * ((D + 3) & ~3) + A) * sizeof(float); }
inline bool ah_shape_ok(int N, int D, int A) { return N >= 1 && D >= 1 && D <= AH_MAXD && A >= 2 && A <= 16; }
inline bool ah_rows_ok(const void* p, int ld, int D) { return p && ld >= ((D + 3) & ~3) && (ld & 3) == 0 && !(reinterpret_cast<uintptr_t>(p) & 15); }

// a kernel that stages [W | b]: its dynamic LDS may pass 64 KB (16 x 1,024 floats + the bias)
template <typename K>
hipError_t ah_allow_lds(K kernel, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

// g [N, 16] | row_term [N] | part [cdiv(N, 16)] x (A D + A), each part a multiple of 4 floats from the start
size_t m2f_aux_head_ws_floats(int N, int D, int A) {
    if (!ah_shape_ok(N, D, A)) return 0;
    return (size_t)N * 16 + (((size_t)N + 3) & ~(size_t)3) + (size_t)m2f_cdiv(N, AH_WROWS) * ((size_t)A * D + A);
}

hipError_t m2f_launch_aux_rows(const AuxHeadArgs& a, hipStream_t stream) {
    if (!ah_shape_ok(a.N, a.D, a.A) || !ah_rows_ok(a.feat, a.ld, a.D) || !a.params || (reinterpret_cast<uintptr_t>(a.params) & 15) || !a.aux_logits ||
        a.ldu < a.A || (a.aux_labels && (!a.labels || !a.hyper || !a.g || !a.row_term || a.C < 1)))
        return hipErrorInvalidValue;
    const size_t lds = ah_lds_bytes(a.A, a.D);
    const dim3 grid(m2f_cdiv(a.N, AH_ROWS));
    auto go = [&](auto kernel) {
        if (hipError_t e = ah_allow_lds(kernel, lds)) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, a.feat, a.N, a.D, a.ld, a.params, a.A, a.labels, a.C, a.class_w, a.aux_labels,
                           a.hyper, a.aux_logits, a.ldu, a.g, a.row_term, a.loss_terms);
        return hipGetLastError();
    };
    return a.D <= 256 ? go(m2f_aux_rows_kernel<1>) : a.D <= 512 ? go(m2f_aux_rows_kernel<2>) : go(m2f_aux_rows_kernel<4>);
}

hipError_t m2f_launch_aux_tail(const float* row_term, const float* loss_terms, int T, float* loss_out, float* scale, int normalise,
                               hipStream_t stream, int accumulate) {
    if (!row_term || !loss_terms || !loss_out || !scale || T < 1) return hipErrorInvalidValue;
    if (accumulate) hipLaunchKernelGGL(m2f_aux_tail_kernel<true>, dim3(1), dim3(256), 0, stream, row_term, loss_terms, T, loss_out, scale, normalise);
    else hipLaunchKernelGGL(m2f_aux_tail_kernel<false>, dim3(1), dim3(256), 0, stream, row_term, loss_terms, T, loss_out, scale, normalise);
    return hipGetLastError();
}

hipError_t m2f_launch_aux_join(float* dh, int ldd, const float* h, int ld, const float* g, int ldg, const float* params, int A, int N, int D,
                               const float* scale, const float* hyper, float gate_scale, int add, int write16, ShadowMap sh, hipStream_t stream) {
    if (!ah_shape_ok(N, D, A) || !ah_rows_ok(dh, ldd, D) || (h && !ah_rows_ok(h, ld, D)) || !g || ldg < A || !params || (reinterpret_cast<uintptr_t>(params) & 15))
        return hipErrorInvalidValue;
    const size_t lds = ah_lds_bytes(A, D);
    const dim3 grid(m2f_cdiv(N, AH_ROWS));
    auto go = [&](auto kernel) {
        if (hipError_t e = ah_allow_lds(kernel, lds)) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, stream, dh, ldd, h, ld, g, ldg, params, A, N, D, scale, hyper, gate_scale, add, write16, sh);
        return hipGetLastError();
    };
    return D <= 256 ? go(m2f_aux_join_kernel<1>) : D <= 512 ? go(m2f_aux_join_kernel<2>) : go(m2f_aux_join_kernel<4>);
}

hipError_t m2f_launch_aux_param_grad(const float* h, int ld, const float* g, int ldg, int A, int N, int D, float* part, const float* scale,
                                     const float* hyper, float* grad, hipStream_t stream) {
    if (!ah_shape_ok(N, D, A) || !ah_rows_ok(h, ld, D) || !g || ldg < A || !part || !grad) return hipErrorInvalidValue;
    const int nblk = m2f_cdiv(N, AH_WROWS), n = A * D + A;
    hipLaunchKernelGGL(m2f_aux_wpart_kernel, dim3(m2f_cdiv(nblk, 4), m2f_cdiv(D, 256)), dim3(256), 0, stream, h, ld, g, ldg, A, N, D, part);
    hipLaunchKernelGGL(m2f_aux_wred_kernel, dim3(m2f_cdiv(n, 256)), dim3(256), 0, stream, part, nblk, n, scale, hyper, grad);
    return hipGetLastError();
}
