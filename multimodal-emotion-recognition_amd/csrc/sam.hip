// Sharpness-aware minimisation (SAM; Foret et al., ICLR 2021) on the flat parameter buffer: optim.FusedAdam(sam_rho=...).
//
//   m2f_sam_finalize_kernel         one workgroup: the float64 partial sums of squares m2f_grad_sumsq left (gradnorm.hip; summed in the
//                                   clip finalize's order) -> record = (||g / den||, c, den, sqrt(sum of squares)), c = rho / (||g / den|| + 1e-12)
//                                   / den: the ONE fp32 coefficient of the perturbation, formed in float64 and rounded once.
//   m2f_sam_perturb_shadow_kernel   bf16 mode: saved <- w, w <- fma(c, g, w), and the W / W^T bf16 shadows of w' - the walk, the tiles and
//                                   the shadow layout (zero fill of a tile's out-of-range elements included) of adam_shadow_body
//                                   (rowops.hip), over items whose 1-D runs end at the tensor's last element: pads are in no tile.
//   m2f_sam_perturb_flat_kernel     fp32 mode (no shadows): the same update over ParamSlices, 16 bytes per lane, four loads in flight.
//   m2f_sam_restore_kernel          w <- saved over ParamSlices: the parameter's bits from before the perturbation.
//
// g, saved and the shadows are streamed once: nontemporal.  w stays cacheable, as in the Adam kernels (the forward's casts, or the
// restore, read it next).  No atomics; the grids come from the table alone and every element is written by one lane: same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// four consecutive gradient elements, fp32 or (G16) bf16, nontemporal
template <bool G16>
__device__ __forceinline__ f32x4 sam_grad4(const void* g, long long o) {
    if constexpr (G16) {
        const u32x2 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(g) + o));
        return (f32x4){__builtin_bit_cast(float, raw.x << 16), __builtin_bit_cast(float, raw.x & 0xFFFF0000u),
                       __builtin_bit_cast(float, raw.y << 16), __builtin_bit_cast(float, raw.y & 0xFFFF0000u)};
    } else {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(static_cast<const float*>(g) + o));
    }
}
template <bool G16>
__device__ __forceinline__ float sam_grad1(const void* g, long long o) {
    if constexpr (G16) return __builtin_bit_cast(float, (uint32_t)static_cast<const uint16_t*>(g)[o] << 16);
    else return static_cast<const float*>(g)[o];
}

// w' = fma(c, g, w), contraction spelled out: every form gives an element the same bits
__device__ __forceinline__ f32x4 sam4(const f32x4& w, const f32x4& g, float c) {
    return (f32x4){__builtin_fmaf(c, g[0], w[0]), __builtin_fmaf(c, g[1], w[1]), __builtin_fmaf(c, g[2], w[2]), __builtin_fmaf(c, g[3], w[3])};
}

__device__ __forceinline__ u32x2 bf16x4(const f32x4& x) {
    u32x2 w;
    w.x = (uint32_t)m2f_bf16_bits(x[0]) | ((uint32_t)m2f_bf16_bits(x[1]) << 16);
    w.y = (uint32_t)m2f_bf16_bits(x[2]) | ((uint32_t)m2f_bf16_bits(x[3]) << 16);
    return w;
}

// record[0] = ||g|| / den, [1] = c, [2] = den, [3] = sqrt(sum of squares).  The partials are summed as m2f_gradnorm_finalize_kernel sums
// them (thread t takes t, t + 1024, ...; wave butterfly; the sixteen wave sums in wave order), so the two records of one buffer agree
// in [3].  A zero gradient gives c = rho / 1e-12 / den, finite: w' = fma(c, 0, w) = w.
__global__ __launch_bounds__(1024) void m2f_sam_finalize_kernel(const double* __restrict__ partial, int n, const float* __restrict__ den_ptr,
                                                                double rho, float* __restrict__ record) {
    __shared__ double red[16];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) a += partial[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) total += red[w];
        const float den = den_ptr ? *den_ptr : 1.0f;
        const double root = sqrt(total), norm = root / (double)den;
        record[0] = (float)norm;
        record[1] = (float)(rho / (norm + 1e-12) / (double)den);
        record[2] = den;
        record[3] = (float)root;
    }
}

template <bool G16>
__global__ __launch_bounds__(256) void m2f_sam_perturb_shadow_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ saved,
                                                                     uint16_t* __restrict__ sh, const AdamItem* __restrict__ items,
                                                                     const int* __restrict__ tile_begin, int n_items, int total_tiles,
                                                                     const float* __restrict__ record) {
    __shared__ float tile[64][65];
    __shared__ int tb[M2F_ADAM_MAX_ITEMS + 1];
    const int tid = threadIdx.x;
    for (int i = tid; i <= n_items; i += 256) tb[i] = tile_begin[i];
    __syncthreads();
    const float c = record[1];
    for (int t = (int)blockIdx.x; t < total_tiles; t += gridDim.x) {
        int lo = 0, hi = n_items - 1;                               // last item whose first tile is <= t (block-uniform)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tb[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const AdamItem it = items[lo];
        const int tl = t - tb[lo];
        if (it.rows == 0) {                                         // 1-D parameter: 4096 consecutive elements per tile, none behind `cols`
            f32x4 pp[4], gg[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                           // all loads of the tile first
                const long long idx = (long long)tl * 4096 + q * 1024 + tid * 4;
                const long long o = it.off + idx;
                pp[q] = (f32x4){0.f, 0.f, 0.f, 0.f}; gg[q] = pp[q];
                if (idx + 4 <= it.cols) {
                    pp[q] = *reinterpret_cast<const f32x4*>(p + o);
                    gg[q] = sam_grad4<G16>(g, o);
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (idx + e < it.cols) { pp[q][e] = p[o + e]; gg[q][e] = sam_grad1<G16>(g, o + e); }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long idx = (long long)tl * 4096 + q * 1024 + tid * 4;
                const long long o = it.off + idx;
                const f32x4 nw = sam4(pp[q], gg[q], c);
                if (idx + 4 <= it.cols) {
                    __builtin_nontemporal_store(pp[q], reinterpret_cast<f32x4*>(saved + o));
                    *reinterpret_cast<f32x4*>(p + o) = nw;
                } else {
#pragma unroll
                    for (int e = 0; e < 3; ++e)
                        if (idx + e < it.cols) { saved[o + e] = pp[q][e]; p[o + e] = nw[e]; }
                }
            }
            continue;
        }
        const int rows = it.rows, cols = it.cols, ldd = (cols + 7) & ~7, ldt = (rows + 7) & ~7;
        const int r0 = (tl / it.tiles_c) << 6, c0 = (tl % it.tiles_c) << 6;
        const int lr = tid >> 4, cl = 4 * (tid & 15), gc = c0 + cl;
        const bool vec = (cols & 3) == 0;                           // then every 4-column group is whole and 16-byte aligned
        f32x4 pp[4], gg[4];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                               // all loads of the tile first, then the arithmetic
            const int gr = r0 + lr + 16 * i;
            in[i] = gr < rows && gc < cols;
            const long long o = it.off + (long long)gr * cols + gc;
            pp[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; gg[i] = pp[i];
            if (in[i]) {
                if (vec) {
                    pp[i] = *reinterpret_cast<const f32x4*>(p + o);
                    gg[i] = sam_grad4<G16>(g, o);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (gc + e < cols) { pp[i][e] = p[o + e]; gg[i][e] = sam_grad1<G16>(g, o + e); }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = lr + 16 * i, gr = r0 + r;
            const f32x4 nw = sam4(pp[i], gg[i], c);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[r][cl + e] = (in[i] && gc + e < cols) ? nw[e] : 0.f;
            if (in[i]) {
                const long long o = it.off + (long long)gr * cols + gc;
                uint16_t* q = sh + it.soff + (long long)gr * ldd + gc;
                if (vec) {
                    __builtin_nontemporal_store(pp[i], reinterpret_cast<f32x4*>(saved + o));
                    *reinterpret_cast<f32x4*>(p + o) = nw;
                    __builtin_nontemporal_store(bf16x4(nw), reinterpret_cast<u32x2*>(q));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (gc + e < cols) { saved[o + e] = pp[i][e]; p[o + e] = nw[e]; q[e] = m2f_bf16_bits(nw[e]); }
                }
            }
        }
        __syncthreads();
        {   // W^T shadow: 8 consecutive source rows of one column per lane = 16 bytes of a dst_t row (as adam_shadow_body)
            const int r8 = tid & 7;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cc = (tid >> 3) + 32 * j;
                const int gcol = c0 + cc, gr0 = r0 + 8 * r8;
                if (gcol < cols && gr0 < ldt) {
                    uint16_t h[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) h[k] = m2f_bf16_bits(tile[8 * r8 + k][cc]);
                    u32x4 w;
                    w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
                    w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
                    __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(sh + it.soff_t + (long long)gcol * ldt + gr0));      // soff_t, ldt: multiples of 8
                }
            }
        }
        __syncthreads();
    }
}

// fp32 mode: slices of at most M2F_PARAM_SLICE elements of one tensor (pads are in no slice); four 16-byte pieces of w and of g per
// lane in flight, twice per slice; the last 1-3 elements of a tensor whose size is no multiple of 4 go one by one.
template <bool G16>
__global__ __launch_bounds__(256) void m2f_sam_perturb_flat_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ saved,
                                                                   const ParamSlice* __restrict__ slices, int n_slices,
                                                                   const float* __restrict__ record) {
    const float c = record[1];
    const int tid = threadIdx.x;
    for (int s = (int)blockIdx.x; s < n_slices; s += (int)gridDim.x) {
        const ParamSlice sl = slices[s];
#pragma unroll 1
        for (int half = 0; half < M2F_PARAM_SLICE / 4096; ++half) {
            f32x4 pp[4], gg[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = ((half * 4 + j) * 256 + tid) * 4;
                const long long o = sl.off + e;                     // tensor offsets are multiples of 64 elements: 16-byte aligned
                pp[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; gg[j] = pp[j];
                if (e + 4 <= sl.n) {
                    pp[j] = *reinterpret_cast<const f32x4*>(p + o);
                    gg[j] = sam_grad4<G16>(g, o);
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (e + k < sl.n) { pp[j][k] = p[o + k]; gg[j][k] = sam_grad1<G16>(g, o + k); }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = ((half * 4 + j) * 256 + tid) * 4;
                const long long o = sl.off + e;
                const f32x4 nw = sam4(pp[j], gg[j], c);
                if (e + 4 <= sl.n) {
                    __builtin_nontemporal_store(pp[j], reinterpret_cast<f32x4*>(saved + o));
                    *reinterpret_cast<f32x4*>(p + o) = nw;
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (e + k < sl.n) { saved[o + k] = pp[j][k]; p[o + k] = nw[k]; }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void m2f_sam_restore_kernel(float* __restrict__ p, const float* __restrict__ saved,
                                                              const ParamSlice* __restrict__ slices, int n_slices) {
    const int tid = threadIdx.x;
    for (int s = (int)blockIdx.x; s < n_slices; s += (int)gridDim.x) {
        const ParamSlice sl = slices[s];
#pragma unroll 1
        for (int half = 0; half < M2F_PARAM_SLICE / 4096; ++half) {
            f32x4 ss[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = ((half * 4 + j) * 256 + tid) * 4;
                const long long o = sl.off + e;
                ss[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (e + 4 <= sl.n) {
                    ss[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(saved + o));
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) if (e + k < sl.n) ss[j][k] = saved[o + k];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = ((half * 4 + j) * 256 + tid) * 4;
                const long long o = sl.off + e;
                if (e + 4 <= sl.n) {
                    *reinterpret_cast<f32x4*>(p + o) = ss[j];
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) if (e + k < sl.n) p[o + k] = ss[j][k];
                }
            }
        }
    }
}

}  // namespace

hipError_t m2f_launch_sam_finalize(const double* partial, int n, const float* den_ptr, double rho, float* record, hipStream_t stream) {
    if (!partial || !record || n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_sam_finalize_kernel, dim3(1), dim3(1024), 0, stream, partial, n, den_ptr, rho, record);
    return hipGetLastError();
}

hipError_t m2f_launch_sam_perturb_shadowed(float* p, const void* g, int g_is_bf16, float* saved, uint16_t* shadow, const AdamItem* items,
                                           const int* tile_begin, int n_items, int total_tiles, const float* record, hipStream_t stream) {
    if (!p || !g || !saved || !shadow || !items || !tile_begin || !record || n_items < 1 || n_items > M2F_ADAM_MAX_ITEMS || total_tiles < 1)
        return hipErrorInvalidValue;
    const int blocks = total_tiles < 256 * 8 ? total_tiles : 256 * 8;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, p, g, saved, shadow, items, tile_begin, n_items, total_tiles, record);
    };
    if (g_is_bf16) go(m2f_sam_perturb_shadow_kernel<true>); else go(m2f_sam_perturb_shadow_kernel<false>);
    return hipGetLastError();
}

hipError_t m2f_launch_sam_perturb_flat(float* p, const void* g, int g_is_bf16, float* saved, const ParamSlice* slices, int n_slices,
                                       const float* record, hipStream_t stream) {
    if (!p || !g || !saved || !slices || !record || n_slices < 0) return hipErrorInvalidValue;
    if (n_slices == 0) return hipSuccess;
    const int blocks = n_slices < 256 * 8 ? n_slices : 256 * 8;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, p, g, saved, slices, n_slices, record); };
    if (g_is_bf16) go(m2f_sam_perturb_flat_kernel<true>); else go(m2f_sam_perturb_flat_kernel<false>);
    return hipGetLastError();
}

hipError_t m2f_launch_sam_restore(float* p, const float* saved, const ParamSlice* slices, int n_slices, hipStream_t stream) {
    if (!p || !saved || !slices || n_slices < 0) return hipErrorInvalidValue;
    if (n_slices == 0) return hipSuccess;
    hipLaunchKernelGGL(m2f_sam_restore_kernel, dim3(n_slices < 256 * 8 ? n_slices : 256 * 8), dim3(256), 0, stream, p, saved, slices, n_slices);
    return hipGetLastError();
}
