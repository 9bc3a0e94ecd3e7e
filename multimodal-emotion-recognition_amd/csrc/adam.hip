// The fused optimizer (optim.FusedAdam / FusedAdamW; reference src/train.py:56) on the flat parameter buffer: thin bodies over the walks
// and element functions of param_walk.h.
//
//   m2f_adam_kernel<G16, EMA>                  the flat update over pads and tensors alike (fp32 mode, one group)
//   m2f_adam_shadow_kernel<G16, EMA>           bf16 mode: the update walked tile by tile, with the bf16 W / W^T shadows of the new values
//   m2f_adam_shadow_dev_kernel                 the same with the step's factors read from device memory: a node of the captured step graph
//   m2f_adam_shadow_grouped_kernel<G16, EMA>   parameter groups: each item with its group's row of the hyper table
//   m2f_adam_slices_kernel<G16, EMA>           parameter groups in fp32 mode (no shadows): ParamSlices, each with its group's row
//   m2f_ema_exchange_kernel                    params <-> ema over ParamSlices
//   m2f_adam_hyper_kernel, m2f_adam_hyper_groups_kernel      the step-dependent factors / the groups' rows into device memory
//
// G16: the gradient buffer holds bf16 (the data-parallel bf16 exchange), everything else stays fp32.
// EMA: one more stream - the average `ema` of the parameters (ema4), read and written once per step like m and v and nontemporal like
// them (8 B per parameter on top of 28), over exactly the elements whose parameter is written; EMA == false is the kernel without it.
// g, m, v are streamed once per step: nontemporal accesses keep them from displacing p (re-read by the bf16 cast that opens the next
// forward) in the L2 / Infinity Cache; measured 0.554 -> 0.524 ms per C3 step for the optimizer part.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "common.h"
#include "ops.h"
#include "param_walk.h"

namespace {

// The Adam update as the walks' Op.  GROUPED: adamw4 with a hyper row (lr / bc1, beta1, beta2, eps, coupled wd, 1 / sqrt(bc2), decay) -
// in the tile walk row item_group[i] of the table `hyt`: the item is the same in every lane of the workgroup, so the row arrives by
// scalar loads and costs no vector register.  NTP: whether the 16-byte load of p is nontemporal (the flat and slice kernels) or plain
// (the shadow-writing ones); element-by-element accesses are plain everywhere.
template <bool G16, bool GROUPED, bool EMA, bool NTP>
struct AdamOp {
    float* __restrict__ p; const void* __restrict__ g; float* __restrict__ m; float* __restrict__ v; float* __restrict__ ema;
    float gs, ema_w;
    float lr_bc1, beta1, beta2, eps, wd, inv_sqrt_bc2, decay;
    const float* __restrict__ hyt; const int* __restrict__ item_group;
    long long base;
    f32x4 pp[4], gg[4], mm[4], vv[4];

    __device__ __forceinline__ void init(float* p_, const void* g_, float* m_, float* v_, const float* gs_ptr, float* ema_, float ema_w_) {
        p = p_; g = g_; m = m_; v = v_; ema = ema_; ema_w = ema_w_;
        gs = gs_ptr ? 1.0f / *gs_ptr : 1.0f;
        base = 0; decay = 1.f;
    }
    __device__ __forceinline__ void row(const float* __restrict__ h) {
        lr_bc1 = h[0]; beta1 = h[1]; beta2 = h[2]; eps = h[3]; wd = h[4]; inv_sqrt_bc2 = h[5]; decay = h[6];
    }
    __device__ __forceinline__ void item(int index, const AdamItem& it) {
        base = it.off;
        if constexpr (GROUPED) row(hyt + 8 * item_group[__builtin_amdgcn_readfirstlane(index)]);
    }
    // a lane outside the matrix (n == 0) loads the item's first piece: a valid address instead of a predicate
    __device__ __forceinline__ void load(int i, long long o, int n, bool vec) {
        const long long a = n ? o : base;
        if (vec) {
            if constexpr (NTP) pp[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + a));
            else pp[i] = *reinterpret_cast<const f32x4*>(p + a);
            gg[i] = param_grad4<G16, false>(g, a);
            mm[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m + a));
            vv[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v + a));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long oe = a + (e < n ? e : 0);
                pp[i][e] = p[oe]; gg[i][e] = param_grad1<G16>(g, oe); mm[i][e] = m[oe]; vv[i][e] = v[oe];
            }
        }
    }
    __device__ __forceinline__ f32x4 finish(int i, long long o, int n, bool vec) {
        if constexpr (GROUPED) adamw4(pp[i], gg[i], mm[i], vv[i], gs, lr_bc1, beta1, beta2, eps, wd, inv_sqrt_bc2, decay);
        else adam4(pp[i], gg[i], mm[i], vv[i], gs, lr_bc1, beta1, beta2, eps, wd, inv_sqrt_bc2);
        if (n) {
            if (vec) {
                *reinterpret_cast<f32x4*>(p + o) = pp[i];
                __builtin_nontemporal_store(mm[i], reinterpret_cast<f32x4*>(m + o));
                __builtin_nontemporal_store(vv[i], reinterpret_cast<f32x4*>(v + o));
                if constexpr (EMA) {
                    f32x4 ee = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ema + o));
                    ema4(ee, pp[i], ema_w);
                    __builtin_nontemporal_store(ee, reinterpret_cast<f32x4*>(ema + o));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) { p[o + e] = pp[i][e]; m[o + e] = mm[i][e]; v[o + e] = vv[i][e]; }
                if constexpr (EMA) {
                    f32x4 ee = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < n) ee[e] = ema[o + e];
                    ema4(ee, pp[i], ema_w);
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < n) ema[o + e] = ee[e];
                }
            }
        }
        return pp[i];
    }
};

template <bool G16, bool EMA>
__global__ __launch_bounds__(256) void m2f_adam_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n4, float lr_bc1, float beta1, float beta2,
                                                       float eps, float wd, float inv_sqrt_bc2, const float* __restrict__ gs_ptr,
                                                       float* __restrict__ ema, float ema_w) {
    AdamOp<G16, false, EMA, true> op;
    op.init(p, g, m, v, gs_ptr, ema, ema_w);
    op.lr_bc1 = lr_bc1; op.beta1 = beta1; op.beta2 = beta2; op.eps = eps; op.wd = wd; op.inv_sqrt_bc2 = inv_sqrt_bc2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        op.load(0, 4 * i, 4, true);
        op.finish(0, 4 * i, 4, true);
    }
}

// see ops.h (AdamItem): tiles [tile_first, total_tiles) of items[0, n_items); the 1-D runs piece by piece, shadow stores plain
template <bool G16, bool EMA>
__global__ __launch_bounds__(256) void m2f_adam_shadow_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, uint16_t* __restrict__ sh,
                                                              const AdamItem* __restrict__ items, const int* __restrict__ tile_begin,
                                                              int n_items, int tile_first, int total_tiles, float lr_bc1, float beta1,
                                                              float beta2, float eps, float wd, float inv_sqrt_bc2,
                                                              const float* __restrict__ gs_ptr, float* __restrict__ ema, float ema_w) {
    AdamOp<G16, false, EMA, false> op;
    op.init(p, g, m, v, gs_ptr, ema, ema_w);
    op.lr_bc1 = lr_bc1; op.beta1 = beta1; op.beta2 = beta2; op.eps = eps; op.wd = wd; op.inv_sqrt_bc2 = inv_sqrt_bc2;
    walk_tiles<false, false>(items, tile_begin, n_items, tile_first, total_tiles, sh, op);
}
// the same update with the step-dependent factors read from device memory (m2f_launch_adam_hyper): a node of the captured step graph
__global__ __launch_bounds__(256) void m2f_adam_shadow_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, uint16_t* __restrict__ sh,
                                                                  const AdamItem* __restrict__ items, const int* __restrict__ tile_begin,
                                                                  int n_items, int total_tiles, const float* __restrict__ hy,
                                                                  const float* __restrict__ gs_ptr) {
    AdamOp<false, false, false, false> op;
    op.init(p, g, m, v, gs_ptr, nullptr, 0.f);
    op.row(hy);
    walk_tiles<false, false>(items, tile_begin, n_items, 0, total_tiles, sh, op);
}

// Parameter groups (optim.FusedAdam(params=[...]), FusedAdamW): the shadow-writing update over the tensors of items[] that some group
// owns, item_group[] (parallel to items[]) their group.  The rows live in device memory (refreshed once per step by
// m2f_adam_hyper_groups_kernel), so this ONE form serves the eager step, the [first, end) ranges of the data-parallel path and a
// captured graph.
template <bool G16, bool EMA>
__global__ __launch_bounds__(256) void m2f_adam_shadow_grouped_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m,
                                                                      float* __restrict__ v, uint16_t* __restrict__ sh,
                                                                      const AdamItem* __restrict__ items, const int* __restrict__ tile_begin,
                                                                      const int* __restrict__ item_group, int n_items, int tile_first,
                                                                      int total_tiles, const float* __restrict__ hyt,
                                                                      const float* __restrict__ gs_ptr, float* __restrict__ ema, float ema_w) {
    AdamOp<G16, true, EMA, false> op;
    op.init(p, g, m, v, gs_ptr, ema, ema_w);
    op.hyt = hyt; op.item_group = item_group;
    walk_tiles<false, false>(items, tile_begin, n_items, tile_first, total_tiles, sh, op);
}

// fp32 mode (no shadows to write): the flat kernel runs over pads and tensors alike and cannot know a group, so the grouped form
// walks SLICES of owned tensors (cut by the host from the parameter map as the gradient norm's are), each with its group's hyper row
// (ParamSlice::tag), piece by piece.
template <bool G16, bool EMA>
__global__ __launch_bounds__(256) void m2f_adam_slices_kernel(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, const ParamSlice* __restrict__ slices, int s0, int s1,
                                                              const float* __restrict__ hyt, const float* __restrict__ gs_ptr,
                                                              float* __restrict__ ema, float ema_w) {
    AdamOp<G16, true, EMA, true> op;
    op.init(p, g, m, v, gs_ptr, ema, ema_w);
    for (int s = s0 + (int)blockIdx.x; s < s1; s += (int)gridDim.x) {
        const ParamSlice sl = slices[s];
        op.row(hyt + 8 * sl.tag);
        walk_slice<1>(sl, op);
    }
}

// optim.FusedAdam.averaged_parameters(): params[i] <-> ema[i] in place over the slices [s0, s1) of whole owned tensors (the list the
// flat grouped kernel walks: pads and the tensors of no group belong to no slice and are not touched).  Run twice, it restores both
// buffers bit for bit.
struct ExchangeOp {
    float* __restrict__ p; float* __restrict__ ema;
    f32x4 pp, ee;
    __device__ __forceinline__ void load(int, long long o, int n, bool vec) {
        if (vec) { pp = *reinterpret_cast<const f32x4*>(p + o); ee = *reinterpret_cast<const f32x4*>(ema + o); }
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) { pp[e] = p[o + e]; ee[e] = ema[o + e]; }
        }
    }
    __device__ __forceinline__ f32x4 finish(int, long long o, int n, bool vec) {
        if (vec) { *reinterpret_cast<f32x4*>(p + o) = ee; *reinterpret_cast<f32x4*>(ema + o) = pp; }
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (e < n) { p[o + e] = ee[e]; ema[o + e] = pp[e]; }
        }
        return ee;
    }
};
__global__ __launch_bounds__(256) void m2f_ema_exchange_kernel(float* __restrict__ p, float* __restrict__ ema,
                                                               const ParamSlice* __restrict__ slices, int s0, int s1) {
    ExchangeOp op;
    op.p = p; op.ema = ema;
    for (int s = s0 + (int)blockIdx.x; s < s1; s += (int)gridDim.x) walk_slice<1>(slices[s], op);
}

// step-dependent factors of the update in device memory (a captured graph cannot take them as kernel arguments): one thread
__global__ void m2f_adam_hyper_kernel(float* __restrict__ h, float lr_bc1, float beta1, float beta2, float eps, float wd, float inv_sqrt_bc2) {
    h[0] = lr_bc1; h[1] = beta1; h[2] = beta2; h[3] = eps; h[4] = wd; h[5] = inv_sqrt_bc2; h[6] = 0.f; h[7] = 0.f;
}

// the hyper table: G rows of 8 floats (lr / bc1, beta1, beta2, eps, coupled wd, 1 / sqrt(bc2), decay, spare), formed by the host and
// passed BY VALUE - no host buffer to keep alive, no sync, and a captured graph that reads the table sees the new rows at its next replay
struct AdamHyperRows { float r[M2F_ADAM_MAX_GROUPS * 8]; };
__global__ __launch_bounds__(M2F_ADAM_MAX_GROUPS * 8) void m2f_adam_hyper_groups_kernel(float* __restrict__ h, int n, const AdamHyperRows rows) {
    const int i = threadIdx.x;
    if (i < n) h[i] = rows.r[i];
}

// the four forms <G16, EMA> of a kernel template: f(G16, EMA) with the two as std::bool_constant values
template <class F>
void adam_forms(bool g16, bool ema, F&& f) {
    if (ema) { if (g16) f(std::true_type{}, std::true_type{}); else f(std::false_type{}, std::true_type{}); }
    else if (g16) f(std::true_type{}, std::false_type{});
    else f(std::false_type{}, std::false_type{});
}

inline int adam_blocks(int64_t work) { return work < 256 * 8 ? (int)work : 256 * 8; }

}  // namespace

hipError_t m2f_launch_adam(float* p, const void* g, int g_is_bf16, float* m, float* v, int64_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                           float* ema, float ema_w, hipStream_t stream) {
    if (n & 3) return hipErrorInvalidValue;      // flat buffers are padded to 64 floats per tensor
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const int64_t n4 = n >> 2;
    adam_forms(g_is_bf16, ema, [&](auto G16, auto EMA) {
        hipLaunchKernelGGL((m2f_adam_kernel<decltype(G16)::value, decltype(EMA)::value>), dim3(adam_blocks((n4 + 255) / 256)), dim3(256), 0,
                           stream, p, g, m, v, n4, (float)(lr / bc1), beta1, beta2, eps, weight_decay, (float)(1.0 / sqrt(bc2)),
                           grad_scale_ptr, ema, ema_w);
    });
    return hipGetLastError();
}

hipError_t m2f_launch_adam_shadowed(float* p, const void* g, int g_is_bf16, float* m, float* v, uint16_t* shadow, const AdamItem* items,
                                    const int* tile_begin, int n_items, int tile_first, int total_tiles, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                                    float* ema, float ema_w, hipStream_t stream) {
    const int n_tiles = total_tiles - tile_first;
    if (n_items < 1 || n_items > M2F_ADAM_MAX_ITEMS || tile_first < 0 || n_tiles < 1 || !items || !tile_begin || !shadow) return hipErrorInvalidValue;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    adam_forms(g_is_bf16, ema, [&](auto G16, auto EMA) {
        hipLaunchKernelGGL((m2f_adam_shadow_kernel<decltype(G16)::value, decltype(EMA)::value>), dim3(adam_blocks(n_tiles)), dim3(256), 0,
                           stream, p, g, m, v, shadow, items, tile_begin, n_items, tile_first, total_tiles, (float)(lr / bc1), beta1, beta2,
                           eps, weight_decay, (float)(1.0 / sqrt(bc2)), grad_scale_ptr, ema, ema_w);
    });
    return hipGetLastError();
}

hipError_t m2f_launch_adam_hyper(float* hyper_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int step, hipStream_t stream) {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);       // as m2f_launch_adam_shadowed computes them
    hipLaunchKernelGGL(m2f_adam_hyper_kernel, dim3(1), dim3(1), 0, stream, hyper_dev, (float)(lr / bc1), beta1, beta2, eps, weight_decay,
                       (float)(1.0 / sqrt(bc2)));
    return hipGetLastError();
}
// the shadow-writing kernel with those factors read from `hyper_dev` (m2f_adam_shadow_dev_kernel: same walk, same arithmetic)
hipError_t m2f_launch_adam_shadowed_dev(float* p, const float* g, float* m, float* v, uint16_t* shadow, const AdamItem* items, const int* tile_begin,
                                        int n_items, int total_tiles, const float* hyper_dev, const float* grad_scale_ptr, hipStream_t stream) {
    if (n_items < 1 || n_items > M2F_ADAM_MAX_ITEMS || total_tiles < 1 || !items || !tile_begin || !shadow || !hyper_dev) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_adam_shadow_dev_kernel, dim3(adam_blocks(total_tiles)), dim3(256), 0, stream, p, g, m, v, shadow, items, tile_begin,
                       n_items, total_tiles, hyper_dev, grad_scale_ptr);
    return hipGetLastError();
}

hipError_t m2f_launch_adam_hyper_groups(float* table_dev, const float* rows_host, int n_groups, hipStream_t stream) {
    if (!table_dev || !rows_host || n_groups < 1 || n_groups > M2F_ADAM_MAX_GROUPS) return hipErrorInvalidValue;
    AdamHyperRows rows;
    for (int i = 0; i < M2F_ADAM_MAX_GROUPS * 8; ++i) rows.r[i] = i < n_groups * 8 ? rows_host[i] : 0.f;
    hipLaunchKernelGGL(m2f_adam_hyper_groups_kernel, dim3(1), dim3(M2F_ADAM_MAX_GROUPS * 8), 0, stream, table_dev, n_groups * 8, rows);
    return hipGetLastError();
}

hipError_t m2f_launch_adam_shadowed_grouped(float* p, const void* g, int g_is_bf16, float* m, float* v, uint16_t* shadow, const AdamItem* items,
                                            const int* tile_begin, const int* item_group, int n_items, int tile_first, int total_tiles,
                                            const float* hyper_table, const float* grad_scale_ptr, float* ema, float ema_w,
                                            hipStream_t stream) {
    const int n_tiles = total_tiles - tile_first;
    if (n_items < 1 || n_items > M2F_ADAM_MAX_ITEMS || tile_first < 0 || n_tiles < 1 || !items || !tile_begin || !item_group || !shadow || !hyper_table)
        return hipErrorInvalidValue;
    adam_forms(g_is_bf16, ema, [&](auto G16, auto EMA) {
        hipLaunchKernelGGL((m2f_adam_shadow_grouped_kernel<decltype(G16)::value, decltype(EMA)::value>), dim3(adam_blocks(n_tiles)), dim3(256),
                           0, stream, p, g, m, v, shadow, items, tile_begin, item_group, n_items, tile_first, total_tiles, hyper_table,
                           grad_scale_ptr, ema, ema_w);
    });
    return hipGetLastError();
}

hipError_t m2f_launch_adam_slices(float* p, const void* g, int g_is_bf16, float* m, float* v, const ParamSlice* slices, int s0, int s1,
                                  const float* hyper_table, const float* grad_scale_ptr, float* ema, float ema_w, hipStream_t stream) {
    if (!p || !g || !m || !v || !slices || !hyper_table || s0 < 0 || s1 < s0) return hipErrorInvalidValue;
    if (s1 == s0) return hipSuccess;
    adam_forms(g_is_bf16, ema, [&](auto G16, auto EMA) {
        hipLaunchKernelGGL((m2f_adam_slices_kernel<decltype(G16)::value, decltype(EMA)::value>), dim3(adam_blocks(s1 - s0)), dim3(256), 0,
                           stream, p, g, m, v, slices, s0, s1, hyper_table, grad_scale_ptr, ema, ema_w);
    });
    return hipGetLastError();
}

hipError_t m2f_launch_ema_exchange(float* p, float* ema, const ParamSlice* slices, int s0, int s1, hipStream_t stream) {
    if (!p || !ema || !slices || s0 < 0 || s1 < s0) return hipErrorInvalidValue;
    if (s1 == s0) return hipSuccess;
    hipLaunchKernelGGL(m2f_ema_exchange_kernel, dim3(adam_blocks(s1 - s0)), dim3(256), 0, stream, p, ema, slices, s0, s1);
    return hipGetLastError();
}
