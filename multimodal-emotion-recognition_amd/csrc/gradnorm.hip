// Global L2 norm of the flat gradient buffer and the clip record the optimizer steps with (torch.nn.utils.clip_grad_norm_'s rule,
// norm type 2).  Two launches, no atomics, float64 sums: the published fp32 values are the same bits on every run, for every grid
// size and on every rank that holds the same buffer.
//
//   m2f_gradnorm_sumsq_kernel     one float64 partial per SLICE: at most M2F_PARAM_SLICE consecutive elements of ONE parameter
//                                 tensor (ops.h ParamSlice, the slice every per-tensor kernel walks: param_tables.hip cuts the tensors
//                                 once, so the 256-byte pads between tensors belong to no slice - the data-parallel bf16 exchange buffer is torch.empty and its pads hold garbage).
//                                 A slice's sum depends on the slice alone: lane t of the workgroup takes the same elements in the
//                                 same order whichever workgroup of whichever grid picks the slice up, the wave / LDS tree is fixed.
//   m2f_gradnorm_finalize_kernel  one workgroup: the partials summed in a fixed order (thread t takes t, t + 1024, ...; then the same
//                                 tree), then norm, clip coefficient and the divisor the Adam kernels read as *grad_scale_ptr.
//
// Why float64: the sum of n squares then carries a relative error of about n * 2^-53 at the very worst (1e-8 at C3's 1e8 elements,
// 4e-15 measured on 4 M values spread over 12 decades) - below half an fp32 ulp - so the fp32 norm is the correctly rounded value up
// to one ulp for any slice order, and the tests need no measured tolerance.  fp32 accumulation is already an ulp off at 4 M elements.
// The float64 FMAs (one per element) are a few microseconds of VALU work at C3; the kernel is bound by reading the gradients once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"
#include "block_sum.h"
#include "param_walk.h"

namespace {

__device__ __forceinline__ float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

// sixteen bytes of gradients: 4 fp32 or 8 bf16 values
template <bool NT>
__device__ __forceinline__ u32x4 load16(const void* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else return *reinterpret_cast<const u32x4*>(p);
}

template <bool G16>
__device__ __forceinline__ void square16(const u32x4& r, double (&acc)[4]) {
    if constexpr (G16) {
        const double a0 = bf16_lo(r.x), a1 = bf16_hi(r.x), a2 = bf16_lo(r.y), a3 = bf16_hi(r.y);
        const double a4 = bf16_lo(r.z), a5 = bf16_hi(r.z), a6 = bf16_lo(r.w), a7 = bf16_hi(r.w);
        acc[0] = __builtin_fma(a0, a0, acc[0]); acc[1] = __builtin_fma(a1, a1, acc[1]);
        acc[2] = __builtin_fma(a2, a2, acc[2]); acc[3] = __builtin_fma(a3, a3, acc[3]);
        acc[0] = __builtin_fma(a4, a4, acc[0]); acc[1] = __builtin_fma(a5, a5, acc[1]);
        acc[2] = __builtin_fma(a6, a6, acc[2]); acc[3] = __builtin_fma(a7, a7, acc[3]);
    } else {
        const f32x4 f = __builtin_bit_cast(f32x4, r);           // (the whole vector: a bit_cast of ONE element of an ext-vector reads element 0)
        const double a0 = f[0], a1 = f[1], a2 = f[2], a3 = f[3];
        acc[0] = __builtin_fma(a0, a0, acc[0]); acc[1] = __builtin_fma(a1, a1, acc[1]);
        acc[2] = __builtin_fma(a2, a2, acc[2]); acc[3] = __builtin_fma(a3, a3, acc[3]);
    }
}

// G16: the buffer holds bf16 (M2FNet.set_grad_bf16, the data-parallel bf16 exchange), same indexing.  NT: nontemporal loads.
// Grid-stride over slices [s0, s1); partial[s] is written by exactly one workgroup.
template <bool G16, bool NT>
__global__ __launch_bounds__(256) void m2f_gradnorm_sumsq_kernel(const void* __restrict__ g, const ParamSlice* __restrict__ slices,
                                                                  int s0, int s1, double* __restrict__ partial) {
    constexpr int V = G16 ? 8 : 4;                               // elements per 16-byte load
    constexpr int ROUNDS = M2F_PARAM_SLICE / (256 * V);          // loads per lane and slice: 8 (fp32), 4 (bf16)
    constexpr int ESZ = G16 ? 2 : 4;
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    int par = 0;
    for (int s = s0 + (int)blockIdx.x; s < s1; s += (int)gridDim.x, par ^= 1) {
        const ParamSlice sl = slices[s];
        const char* base = static_cast<const char*>(g) + sl.off * ESZ;          // tensor offsets are multiples of 64 elements: 16-byte aligned
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (sl.n == M2F_PARAM_SLICE) {                           // whole slice (block-uniform): every load first, then the arithmetic
            u32x4 r[ROUNDS];
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) r[j] = load16<NT>(base + ((size_t)j * 256 + tid) * 16);
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) square16<G16>(r[j], acc);
        } else {                                                 // the tail of a tensor: nothing at or beyond element n is read
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const int e = (j * 256 + tid) * V;
                if (e + V <= sl.n) {
                    square16<G16>(load16<NT>(base + (size_t)e * ESZ), acc);
                } else {
                    for (int k = e; k < sl.n; ++k) {
                        const double a = (double)param_grad1<G16>(g, sl.off + k);
                        acc[0] = __builtin_fma(a, a, acc[0]);
                    }
                }
            }
        }
        const double t = block_sum<4>((acc[0] + acc[1]) + (acc[2] + acc[3]), red[par]);      // (red[par ^ 1] is free again after this barrier)
        if (tid == 0) partial[s] = t;
    }
}

// record[0] = norm, [1] = coef, [2] = divisor, [3] = sqrt(sum of squares) before the division by den.  Everything in float64, each value
// rounded ONCE to fp32; coef is computed from the rounded norm and the divisor from the rounded coef, so the record is consistent
// with itself: a reader that re-evaluates the formulas in float64 from the published values gets the published bits back.
// A non-finite norm stays non-finite through coef and divisor (no min / clamp that would drop a NaN).
__global__ __launch_bounds__(1024) void m2f_gradnorm_finalize_kernel(const double* __restrict__ partial, int n,
                                                                     const float* __restrict__ den_ptr, double max_norm,
                                                                     float* __restrict__ record) {
    __shared__ double red[16];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) a += partial[i];
    const double total = block_sum<16>(a, red);
    if (threadIdx.x == 0) {
        const float den = den_ptr ? *den_ptr : 1.0f;
        const double root = sqrt(total);
        const float norm = (float)(root / (double)den);
        const double c = max_norm / ((double)norm + 1e-6);
        const float coef = (c >= 1.0) ? 1.0f : (float)c;                    // NaN -> NaN
        record[0] = norm;
        record[1] = coef;
        record[2] = (coef == 1.0f) ? den : (float)((double)den / (double)coef);
        record[3] = (float)root;
    }
}

}  // namespace

hipError_t m2f_launch_grad_sumsq(const void* g, int g_is_bf16, const ParamSlice* slices, int s0, int s1, double* partial, int grid,
                                 int nontemporal, hipStream_t stream) {
    if (!g || !slices || !partial || s0 < 0 || s1 < s0 || (reinterpret_cast<uintptr_t>(g) & 15)) return hipErrorInvalidValue;
    if (s1 == s0) return hipSuccess;
    // memory-bound: at most 2,048 workgroups, the rest of the slices by grid stride (the grid decides who sums a slice, never what the sum is)
    const int blocks = (grid > 0 ? grid : 2048) < (s1 - s0) ? (grid > 0 ? grid : 2048) : (s1 - s0);
#define M2F_GN_LAUNCH(G16, NT) \
    hipLaunchKernelGGL((m2f_gradnorm_sumsq_kernel<G16, NT>), dim3(blocks), dim3(256), 0, stream, g, slices, s0, s1, partial)
    if (g_is_bf16) { if (nontemporal) M2F_GN_LAUNCH(true, true); else M2F_GN_LAUNCH(true, false); }
    else           { if (nontemporal) M2F_GN_LAUNCH(false, true); else M2F_GN_LAUNCH(false, false); }
#undef M2F_GN_LAUNCH
    return hipGetLastError();
}

hipError_t m2f_launch_grad_norm_finalize(const double* partial, int n, const float* den_ptr, double max_norm, float* record,
                                         hipStream_t stream) {
    if (!partial || !record || n < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_gradnorm_finalize_kernel, dim3(1), dim3(1024), 0, stream, partial, n, den_ptr, max_norm, record);
    return hipGetLastError();
}
