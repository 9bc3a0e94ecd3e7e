// Adversarial training on the input embeddings (FGM, Miyato et al. 2017; PGD, Madry et al. 2018; FreeLB, Zhu et al. 2020): the ascent
// step on the perturbation of one modality's token rows, on the device.
//
// Definition (AdvArgs, ops.h).  Row t of x_clean / g / delta / x has width d and row stride ld (a multiple of 4 floats, >= d rounded up
// to 4: 16-byte aligned rows); skip[t] != 0: the row is padding - never read for a norm, never written.  (epsilon, step) = hyper[0 .. 1],
// read on the device.  ||.|| is the L2 norm of the row (norm kind 0, "utterance") or of all rows that are not skipped (1, "batch"):
//   u      = g / ||g||
//   cand   = delta + step * u                      (||g|| == 0 or not finite: cand = delta)
//   delta' = cand * min(1, epsilon / ||cand||)     (||cand|| == 0: delta' = cand)
//   x      = x_clean + delta'                      (one fp32 add: x == x_clean + delta' bit for bit)
// Columns d .. ld - 1 are never written and never enter a sum.  g NULL: the gradient is zero (the projection alone).
//
// Arithmetic.  Every sum of squares is float64 (block_sum.h: a lane's elements in column order, then the 64-lane butterfly): a norm has
// one fixed order.  step / ||g|| and epsilon / ||cand|| are formed in float64 and rounded ONCE to fp32; an element is then
// cand = fma(a, g, delta), delta' = cand * s, x = x_clean + delta' in fp32: ||delta'|| <= epsilon * (1 + 2^-22).
//
// Launches.
//   rows<V>    norm kind 0: one wave per row, four rows per workgroup, V = 1, 2 or 4 16-byte pieces per lane and array (d <= 1,024): the
//              row's loads of g, delta and x_clean are all issued before the first arithmetic and the row stays in registers
//   rows_loop  the same for any d: three passes over the row (the second and third hit the L2)
//   partial    norm kind 1, first launch: per slice of ADV_SLICE consecutive rows (a slicing that follows from T alone) the float64 sums
//              of g^2, delta^2 and delta . g over the rows that are not skipped -> partial[3 * slice ..]
//   rows / rows_loop with BATCH: second launch: every workgroup adds the partials in index order (thread t takes t, t + 256, ...; then
//              block_sum), and ||cand||^2 = sum delta^2 + 2 (step / ||g||) sum delta . g + step^2 follows by algebra - no third pass
//   init       delta[t, c] = scale * (2 * (h >> 8) * 2^-24 - 1), h the dropout hash (common.h) of element t * d + c under the caller's
//              site; scale = fp32(init_mag / sqrt(d)) from the host
// No atomics, every element is written by one lane, the grids follow from T alone: same bits on every run.  Plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"
#include "block_sum.h"

namespace {

constexpr int ADV_SLICE = 16;        // rows per partial of the batch norm: four per wave

__device__ __forceinline__ double adv_sq(const f32x4& v, double acc) {
    const double a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];
    acc = __builtin_fma(a0, a0, acc); acc = __builtin_fma(a1, a1, acc);
    acc = __builtin_fma(a2, a2, acc); acc = __builtin_fma(a3, a3, acc);
    return acc;
}
__device__ __forceinline__ double adv_dot(const f32x4& v, const f32x4& w, double acc) {
    acc = __builtin_fma((double)v[0], (double)w[0], acc); acc = __builtin_fma((double)v[1], (double)w[1], acc);
    acc = __builtin_fma((double)v[2], (double)w[2], acc); acc = __builtin_fma((double)v[3], (double)w[3], acc);
    return acc;
}
// A row as a buffer descriptor over its whole 16-byte pieces (common.h: a load outside the range reads zeros and touches no memory; a null
// or dead row has no range at all), so that every load of a row is issued unconditionally - a guarded plain load costs a wait per guard
__device__ __forceinline__ m2f_rsrc_t adv_row(const float* base, size_t off, int d, bool live) {
    return m2f_make_rsrc(base && live ? base + off : nullptr, (uint32_t)((d + 3) >> 2) * 16u);
}
// the 16 bytes behind column k, the columns from d on SELECTED to 0 (a piece that straddles d holds pad columns)
__device__ __forceinline__ f32x4 adv_load(m2f_rsrc_t row, int k, int d) {
    f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(row, k * 4, 0, 0));
    v[0] = k + 0 < d ? v[0] : 0.f; v[1] = k + 1 < d ? v[1] : 0.f; v[2] = k + 2 < d ? v[2] : 0.f; v[3] = k + 3 < d ? v[3] : 0.f;
    return v;
}
// ... and a store that never touches a pad column
__device__ __forceinline__ void adv_store(float* __restrict__ row, int k, int d, const f32x4& v) {
    if (k + 3 < d) *reinterpret_cast<f32x4*>(row + k) = v;
    else {
#pragma unroll
        for (int e = 0; e < 3; ++e) if (k + e < d) row[k + e] = v[e];
    }
}

// The two coefficients of a row (or of the batch) from its float64 sums: cand = move ? fma(a, g, delta) : delta, delta' = clip ? cand * s : cand
struct AdvCoef { float a, s; bool move, clip; };
__device__ __forceinline__ bool adv_move(double sgg) { const double ng = sqrt(sgg); return ng > 0.0 && ng <= 1.7976931348623157e308; }
__device__ __forceinline__ float adv_step_coef(double sgg, float step) { return (float)((double)step / sqrt(sgg)); }
__device__ __forceinline__ void adv_clip(AdvCoef& c, double scc, float epsilon) {
    const double nc = sqrt(scc);
    c.clip = nc > (double)epsilon;                      // (a NaN norm clips nothing: the row keeps its candidate)
    c.s = c.clip ? (float)((double)epsilon / nc) : 1.f;
}
__device__ __forceinline__ f32x4 adv_cand(const AdvCoef& c, const f32x4& g, const f32x4& dl) {
    f32x4 r = dl;
    if (c.move) { r[0] = fmaf(c.a, g[0], dl[0]); r[1] = fmaf(c.a, g[1], dl[1]); r[2] = fmaf(c.a, g[2], dl[2]); r[3] = fmaf(c.a, g[3], dl[3]); }
    return r;
}

// Batch norm, second launch: the partials in index order -> the batch's coefficients, the same in every workgroup.  All 256 threads.
__device__ __forceinline__ AdvCoef adv_batch_coef(const double* __restrict__ partial, int n_slices, float epsilon, float step) {
    __shared__ double red[3][4];
    __shared__ double tot[3];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_slices; i += 256) {
        acc[0] += partial[3 * i]; acc[1] += partial[3 * i + 1]; acc[2] += partial[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double t = block_sum<4>(acc[j], red[j]);
        if (threadIdx.x == 0) tot[j] = t;
    }
    __syncthreads();
    const double sgg = tot[0], sdd = tot[1], sdg = tot[2];
    AdvCoef c;
    c.move = adv_move(sgg);
    c.a = c.move ? adv_step_coef(sgg, step) : 0.f;
    // ||delta + a g||^2 with a = step / ||g||: the cross term and step^2 (a^2 ||g||^2 = step^2); rounding may leave it a hair below zero
    double scc = sdd;
    if (c.move) scc = sdd + 2.0 * ((double)step / sqrt(sgg)) * sdg + (double)step * (double)step;
    adv_clip(c, scc > 0.0 ? scc : (scc == scc ? 0.0 : scc), epsilon);
    return c;
}

// d <= 256 * V: the row in registers
template <int V, bool BATCH>
__global__ __launch_bounds__(256) void m2f_adv_rows_kernel(AdvArgs a) {
    const float epsilon = a.hyper[0], step = a.hyper[1];
    AdvCoef c{0.f, 1.f, false, false};
    const int lane = threadIdx.x & 63, t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const bool live = t < a.T && !a.skip[t < a.T ? t : 0];                 // (wave-uniform)
    const size_t off = (size_t)(live ? t : 0) * a.ld;
    const m2f_rsrc_t gr = adv_row(a.g, off, a.d, live), dr = adv_row(a.delta, off, a.d, live), xr = adv_row(a.x_clean, off, a.d, live);
    f32x4 g[V], dl[V], xc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = adv_load(gr, 4 * (lane + 64 * j), a.d);
#pragma unroll
    for (int j = 0; j < V; ++j) dl[j] = adv_load(dr, 4 * (lane + 64 * j), a.d);
#pragma unroll
    for (int j = 0; j < V; ++j) xc[j] = adv_load(xr, 4 * (lane + 64 * j), a.d);
    __builtin_amdgcn_sched_barrier(0);                                     // (all 3 V loads issued: hipcc otherwise sinks delta's and x_clean's behind the first sum)
    if constexpr (BATCH) c = adv_batch_coef(a.partial, a.n_slices, epsilon, step);      // (the row's loads travel under the partials' sum)
    if (!live) return;                                                     // (no barrier follows)
    if constexpr (!BATCH) {
        double sgg = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) sgg = adv_sq(g[j], sgg);
        sgg = wave_sum(sgg);
        c.move = adv_move(sgg);
        c.a = c.move ? adv_step_coef(sgg, step) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) dl[j] = adv_cand(c, g[j], dl[j]);
    if constexpr (!BATCH) {
        double scc = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) scc = adv_sq(dl[j], scc);
        adv_clip(c, wave_sum(scc), epsilon);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int k = 4 * (lane + 64 * j);
        if (k < a.d) {
            const f32x4 nd = c.clip ? dl[j] * c.s : dl[j];
            adv_store(a.delta + off, k, a.d, nd);
            adv_store(a.x + off, k, a.d, xc[j] + nd);
        }
    }
}

// any d: the row in passes
template <bool BATCH>
__global__ __launch_bounds__(256) void m2f_adv_rows_loop_kernel(AdvArgs a) {
    const float epsilon = a.hyper[0], step = a.hyper[1];
    AdvCoef c{0.f, 1.f, false, false};
    if constexpr (BATCH) c = adv_batch_coef(a.partial, a.n_slices, epsilon, step);
    const int lane = threadIdx.x & 63, t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (t >= a.T || a.skip[t]) return;                                     // (wave-uniform; no barrier follows)
    const size_t off = (size_t)t * a.ld;
    const m2f_rsrc_t gr = adv_row(a.g, off, a.d, true), dr = adv_row(a.delta, off, a.d, true), xr = adv_row(a.x_clean, off, a.d, true);
    if constexpr (!BATCH) {
        double sgg = 0.0;
        for (int k = 4 * lane; k < a.d; k += 256) sgg = adv_sq(adv_load(gr, k, a.d), sgg);
        sgg = wave_sum(sgg);
        c.move = adv_move(sgg);
        c.a = c.move ? adv_step_coef(sgg, step) : 0.f;
        double scc = 0.0;
        for (int k = 4 * lane; k < a.d; k += 256) scc = adv_sq(adv_cand(c, adv_load(gr, k, a.d), adv_load(dr, k, a.d)), scc);
        adv_clip(c, wave_sum(scc), epsilon);
    }
    for (int k = 4 * lane; k < a.d; k += 256) {
        const f32x4 g = adv_load(gr, k, a.d), dl = adv_load(dr, k, a.d), xc = adv_load(xr, k, a.d);
        const f32x4 cd = adv_cand(c, g, dl);
        const f32x4 nd = c.clip ? cd * c.s : cd;
        adv_store(a.delta + off, k, a.d, nd);
        adv_store(a.x + off, k, a.d, xc + nd);
    }
}

// Batch norm, first launch: workgroup = slice, wave w takes rows 4 w .. 4 w + 3 of it in order, a lane its columns in order
__global__ __launch_bounds__(256) void m2f_adv_partial_kernel(AdvArgs a) {
    __shared__ double red[3][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, slice = blockIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < 4; ++r) {
        const int t = slice * ADV_SLICE + 4 * wv + r;
        if (t >= a.T || a.skip[t]) continue;                               // (wave-uniform)
        const size_t off = (size_t)t * a.ld;
        const m2f_rsrc_t gr = adv_row(a.g, off, a.d, true), dr = adv_row(a.delta, off, a.d, true);
        for (int k = 4 * lane; k < a.d; k += 256) {
            const f32x4 g = adv_load(gr, k, a.d), dl = adv_load(dr, k, a.d);
            acc[0] = adv_sq(g, acc[0]); acc[1] = adv_sq(dl, acc[1]); acc[2] = adv_dot(dl, g, acc[2]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double s = block_sum<4>(acc[j], red[j]);
        if (threadIdx.x == 0) a.partial[3 * (size_t)slice + j] = s;
    }
}

// the uniform start: one wave per row, a lane its columns; rows that are skipped keep their bits
__global__ __launch_bounds__(256) void m2f_adv_init_kernel(float* __restrict__ delta, int T, int d, int ld, const uint8_t* __restrict__ skip,
                                                           float scale, const uint32_t* __restrict__ rng, uint32_t site) {
    const int lane = threadIdx.x & 63, t = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (t >= T || skip[t]) return;
    const uint32_t key = m2f_site_key(rng, site);
    for (int col = lane; col < d; col += 64) {
        const uint32_t idx = (uint32_t)t * (uint32_t)d + (uint32_t)col;
        uint32_t h = m2f_mix32(idx * 0x9E3779B1U + key);                   // (m2f_keep's hash, common.h)
        h = m2f_mix32(h ^ (key >> 7) ^ 0x68e31da4U);
        const float u = (float)(h >> 8) * 1.1920928955078125e-07f - 1.0f;  // 2 * (h >> 8) * 2^-24 - 1: exact in fp32
        delta[(size_t)t * ld + col] = scale * u;
    }
}

}  // namespace

int m2f_adv_slices(int T) { return (T + ADV_SLICE - 1) / ADV_SLICE; }

hipError_t m2f_launch_adv_ascend(const AdvArgs& a, int batch_norm, hipStream_t stream) {
    if (!a.x_clean || !a.delta || !a.x || !a.skip || !a.hyper || a.T < 1 || a.d < 1 || (a.ld & 3) || a.ld < ((a.d + 3) & ~3)) return hipErrorInvalidValue;
    if (batch_norm && !a.partial) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.x_clean) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.delta) | reinterpret_cast<uintptr_t>(a.x)) & 15)
        return hipErrorInvalidValue;
    AdvArgs b = a;
    b.n_slices = m2f_adv_slices(a.T);
    if (batch_norm) hipLaunchKernelGGL(m2f_adv_partial_kernel, dim3(b.n_slices), dim3(256), 0, stream, b);
    const dim3 grid((a.T + 3) / 4), block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, stream, b); };
    if (batch_norm) {
        if (a.d <= 256) go(m2f_adv_rows_kernel<1, true>); else if (a.d <= 512) go(m2f_adv_rows_kernel<2, true>);
        else if (a.d <= 1024) go(m2f_adv_rows_kernel<4, true>); else go(m2f_adv_rows_loop_kernel<true>);
    } else {
        if (a.d <= 256) go(m2f_adv_rows_kernel<1, false>); else if (a.d <= 512) go(m2f_adv_rows_kernel<2, false>);
        else if (a.d <= 1024) go(m2f_adv_rows_kernel<4, false>); else go(m2f_adv_rows_loop_kernel<false>);
    }
    return hipGetLastError();
}

hipError_t m2f_launch_adv_init(float* delta, int T, int d, int ld, const uint8_t* skip, float scale, const uint32_t* rng, uint32_t site,
                               hipStream_t stream) {
    if (!delta || !skip || !rng || T < 1 || d < 1 || ld < d) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_adv_init_kernel, dim3((T + 3) / 4), dim3(256), 0, stream, delta, T, d, ld, skip, scale, rng, site);
    return hipGetLastError();
}
