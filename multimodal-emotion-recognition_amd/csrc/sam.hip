// Sharpness-aware minimisation (SAM; Foret et al., ICLR 2021) on the flat parameter buffer: optim.FusedAdam(sam_rho=...).
//
//   m2f_sam_finalize_kernel         one workgroup: the float64 partial sums of squares m2f_grad_sumsq left (gradnorm.hip; summed in the
//                                   clip finalize's order) -> record = (||g / den||, c, den, sqrt(sum of squares)), c = rho / (||g / den|| + 1e-12)
//                                   / den: the ONE fp32 coefficient of the perturbation, formed in float64 and rounded once.
//   m2f_sam_perturb_shadow_kernel   bf16 mode: saved <- w, w <- fma(c, g, w), and the W / W^T bf16 shadows of w' - param_walk.h's tile walk
//                                   and shadow writer (the Adam kernels'), over items whose 1-D runs end at the tensor's last element:
//                                   pads are in no tile.
//   m2f_sam_perturb_flat_kernel     fp32 mode (no shadows): the same update over ParamSlices, four pieces per lane in flight.
//   m2f_sam_restore_kernel          w <- saved over ParamSlices: the parameter's bits from before the perturbation.
//
// g, saved and the shadows are streamed once: nontemporal.  w stays cacheable, as in the Adam kernels (the forward's casts, or the
// restore, read it next).  No atomics; the grids come from the table alone and every element is written by one lane: same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"
#include "block_sum.h"
#include "param_walk.h"

namespace {

// record[0] = ||g|| / den, [1] = c, [2] = den, [3] = sqrt(sum of squares).  The partials are summed as m2f_gradnorm_finalize_kernel sums
// them (thread t takes t, t + 1024, ...; block_sum<16>), so the two records of one buffer agree in [3].  A zero gradient gives
// c = rho / 1e-12 / den, finite: w' = fma(c, 0, w) = w.
__global__ __launch_bounds__(1024) void m2f_sam_finalize_kernel(const double* __restrict__ partial, int n, const float* __restrict__ den_ptr,
                                                                double rho, float* __restrict__ record) {
    __shared__ double red[16];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) a += partial[i];
    const double total = block_sum<16>(a, red);
    if (threadIdx.x == 0) {
        const float den = den_ptr ? *den_ptr : 1.0f;
        const double root = sqrt(total), norm = root / (double)den;
        record[0] = (float)norm;
        record[1] = (float)(rho / (norm + 1e-12) / (double)den);
        record[2] = den;
        record[3] = (float)root;
    }
}

// The perturbation as the walks' Op: saved <- w (nontemporal), w <- sam4 (cacheable), all loads of a batch before the arithmetic; a lane
// outside the matrix loads nothing and carries zeros.
template <bool G16>
struct SamOp {
    float* __restrict__ p; const void* __restrict__ g; float* __restrict__ saved;
    float c;
    f32x4 pp[4], gg[4];
    __device__ __forceinline__ void item(int, const AdamItem&) {}
    __device__ __forceinline__ void load(int i, long long o, int n, bool vec) {
        pp[i] = (f32x4){0.f, 0.f, 0.f, 0.f}; gg[i] = pp[i];
        if (n) {
            if (vec) {
                pp[i] = *reinterpret_cast<const f32x4*>(p + o);
                gg[i] = param_grad4<G16, true>(g, o);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) { pp[i][e] = p[o + e]; gg[i][e] = param_grad1<G16>(g, o + e); }
            }
        }
    }
    __device__ __forceinline__ f32x4 finish(int i, long long o, int n, bool vec) {
        const f32x4 nw = sam4(pp[i], gg[i], c);
        if (n) {
            if (vec) {
                __builtin_nontemporal_store(pp[i], reinterpret_cast<f32x4*>(saved + o));
                *reinterpret_cast<f32x4*>(p + o) = nw;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) { saved[o + e] = pp[i][e]; p[o + e] = nw[e]; }
            }
        }
        return nw;
    }
};

// shadow stores nontemporal (the next forward's GEMMs read them from memory), the 1-D runs four loads at a time
template <bool G16>
__global__ __launch_bounds__(256) void m2f_sam_perturb_shadow_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ saved,
                                                                     uint16_t* __restrict__ sh, const AdamItem* __restrict__ items,
                                                                     const int* __restrict__ tile_begin, int n_items, int total_tiles,
                                                                     const float* __restrict__ record) {
    SamOp<G16> op;
    op.p = p; op.g = g; op.saved = saved; op.c = record[1];
    walk_tiles<true, true>(items, tile_begin, n_items, 0, total_tiles, sh, op);
}

template <bool G16>
__global__ __launch_bounds__(256) void m2f_sam_perturb_flat_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ saved,
                                                                   const ParamSlice* __restrict__ slices, int n_slices,
                                                                   const float* __restrict__ record) {
    SamOp<G16> op;
    op.p = p; op.g = g; op.saved = saved; op.c = record[1];
    for (int s = (int)blockIdx.x; s < n_slices; s += (int)gridDim.x) walk_slice<4>(slices[s], op);
}

struct RestoreOp {
    float* __restrict__ p; const float* __restrict__ saved;
    f32x4 ss[4];
    __device__ __forceinline__ void load(int i, long long o, int n, bool vec) {
        if (vec) ss[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(saved + o));
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) ss[i][e] = saved[o + e];
        }
    }
    __device__ __forceinline__ f32x4 finish(int i, long long o, int n, bool vec) {
        if (vec) *reinterpret_cast<f32x4*>(p + o) = ss[i];
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) p[o + e] = ss[i][e];
        }
        return ss[i];
    }
};
__global__ __launch_bounds__(256) void m2f_sam_restore_kernel(float* __restrict__ p, const float* __restrict__ saved,
                                                              const ParamSlice* __restrict__ slices, int n_slices) {
    RestoreOp op;
    op.p = p; op.saved = saved;
    for (int s = (int)blockIdx.x; s < n_slices; s += (int)gridDim.x) walk_slice<4>(slices[s], op);
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
