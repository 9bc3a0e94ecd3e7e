// How a kernel walks the flat parameter buffer, written ONCE: the gradient loaders, the element functions of the optimizer (adam4, adamw4,
// ema4, sam4), the walk over 64 x 64 tiles with the SINGLE writer of the bf16 W / W^T parameter shadows the GEMMs read, and the walk
// over ParamSlices.  adam.hip, sam.hip, rowops.hip (m2f_cast_items_kernel), gradnorm.hip (the loader) and gemm_p8.h (adam4 in the
// weight-gradient epilogue) are thin bodies over it: the equalities the suite promises (every form of the update gives an element the
// same bits; SAM's shadows are the Adam kernel's of the same values) hold because the statements ARE the same.
// tests/golden/optimizer_kernel_bits.npz holds the bits from before the copies became this header.
//
// The bits must not depend on who includes the header: every element function turns fp contraction off ITSELF and spells its
// contractions out (the pragma at the start of its body; the setting travels with the inlined instructions).
//
// The walks take the per-piece work as a functor and never ask which kernel called them.  A PIECE is four consecutive elements at flat
// offset o of which the first n (0..4) exist; `vec` says that a piece with n == 4 may be accessed as 16 bytes.  An Op has
//     void  item(int index, const AdamItem& it)                 tile walk only, block-uniform: the tile's item (a group's hyper row ...)
//     void  load(int i, long long o, int n, bool vec)           issue the loads of piece i of the batch
//     f32x4 finish(int i, long long o, int n, bool vec)         arithmetic and stores of piece i -> the new parameter values
// and keeps to itself what differs between kernels: which streams exist (m / v / ema / saved), each stream's cache hint, the hyper row,
// and what it loads for the lanes of a tile outside the matrix (n == 0: finish is still called, its values are not used).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---- loaders and the pack ---------------------------------------------------------------------------------------------------------------
// four consecutive gradient elements from the fp32 buffer (nontemporal: streamed once) or (G16: M2FNet.set_grad_bf16, the data-parallel
// bf16 exchange) from the bf16 buffer, same indexing; NT16: the bf16 load's cache hint, the caller's choice
template <bool G16, bool NT16>
__device__ __forceinline__ f32x4 param_grad4(const void* g, long long o) {
    if constexpr (G16) {
        const u32x2* q = reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(g) + o);
        u32x2 raw;
        if constexpr (NT16) raw = __builtin_nontemporal_load(q); else raw = *q;
        return (f32x4){__builtin_bit_cast(float, raw.x << 16), __builtin_bit_cast(float, raw.x & 0xFFFF0000u),
                       __builtin_bit_cast(float, raw.y << 16), __builtin_bit_cast(float, raw.y & 0xFFFF0000u)};
    } else {
        return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(static_cast<const float*>(g) + o));
    }
}
template <bool G16>
__device__ __forceinline__ float param_grad1(const void* g, long long o) {
    if constexpr (G16) return __builtin_bit_cast(float, (uint32_t)static_cast<const uint16_t*>(g)[o] << 16);
    else return static_cast<const float*>(g)[o];
}

// four floats -> four bf16 (round to nearest even), 8 bytes
__device__ __forceinline__ u32x2 param_bf16x4(const f32x4& x) {
    u32x2 w;
    w.x = (uint32_t)m2f_bf16_bits(x[0]) | ((uint32_t)m2f_bf16_bits(x[1]) << 16);
    w.y = (uint32_t)m2f_bf16_bits(x[2]) | ((uint32_t)m2f_bf16_bits(x[3]) << 16);
    return w;
}
template <bool NT, typename V>
__device__ __forceinline__ void param_store(V* q, const V& x) {
    if constexpr (NT) __builtin_nontemporal_store(x, q); else *q = x;
}

// ---- element functions ------------------------------------------------------------------------------------------------------------------
// Adam update of four consecutive elements (registers in, registers out).  Every optimizer kernel goes through this one function and
// its contractions are spelled out: left to the compiler (contract(fast)) the flat kernel and the shadow-writing kernel fused
// `g * gs + wd * p` differently once one of them became a template, and a data-parallel run (bucket-wise shadow-writing steps) drifted
// from the single-process run by an ulp per step.
__device__ __forceinline__ void adam4(f32x4& pp, const f32x4& gg, f32x4& mm, f32x4& vv, float gs, float lr_bc1, float beta1,
                                      float beta2, float eps, float wd, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gr = __builtin_fmaf(gg[e], gs, wd * pp[e]);     // coupled L2 (Adam, not AdamW)
        mm[e] = __builtin_fmaf(beta1, mm[e], (1.f - beta1) * gr);
        vv[e] = __builtin_fmaf(beta2, vv[e], ((1.f - beta2) * gr) * gr);
        const float denom = __builtin_fmaf(sqrtf(vv[e]), inv_sqrt_bc2, eps);
        pp[e] = __builtin_fmaf(-lr_bc1, mm[e] / denom, pp[e]);
    }
}

// The grouped kernels' update (one hyper row per parameter group, m2f_adam_hyper_groups_kernel): torch.optim.AdamW multiplies the
// parameter by `decay` = 1 - lr * weight_decay first (torch's param.mul_: ONE rounded fp32 multiply; the row of a decoupled group holds
// a coupled weight decay of 0), then the statements of adam4.  A coupled group's row holds decay = 1.0f, an exact multiply: its result
// is adam4's, bit for bit.
__device__ __forceinline__ void adamw4(f32x4& pp, const f32x4& gg, f32x4& mm, f32x4& vv, float gs, float lr_bc1, float beta1,
                                       float beta2, float eps, float wd, float inv_sqrt_bc2, float decay) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) pp[e] = pp[e] * decay;
    adam4(pp, gg, mm, vv, gs, lr_bc1, beta1, beta2, eps, wd, inv_sqrt_bc2);
}

// Exponential moving average of the weights (optim.FusedAdam(ema_decay=...); torch.optim.swa_utils.AveragedModel.update_parameters with
// get_ema_multi_avg_fn(decay): e.lerp_(p, 1 - decay)) of four consecutive elements, applied to the parameter adam4 / adamw4 has just
// produced.  w = (float)(1 - decay_t), formed in double on the host, the same for every launch of one step.  w == 1 is the first
// update (torch's n_averaged == 0 copy): the average becomes the parameter's bits, whatever the buffer held.
__device__ __forceinline__ void ema4(f32x4& ee, const f32x4& pp, float w) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) ee[e] = (w == 1.0f) ? pp[e] : __builtin_fmaf(w, pp[e] - ee[e], ee[e]);
}

// SAM's perturbation w' = fma(c, g, w)
__device__ __forceinline__ f32x4 sam4(const f32x4& w, const f32x4& g, float c) {
#pragma clang fp contract(off)
    return (f32x4){__builtin_fmaf(c, g[0], w[0]), __builtin_fmaf(c, g[1], w[1]), __builtin_fmaf(c, g[2], w[2]), __builtin_fmaf(c, g[3], w[3])};
}

// ---- the tile walk (ops.h AdamItem) -----------------------------------------------------------------------------------------------------
// (1) the prefix array tile_begin[0 .. n_items] (absolute tile numbers) into LDS: tb = M2F_ADAM_MAX_ITEMS + 1 ints
__device__ __forceinline__ void walk_prefix(int* tb, const int* __restrict__ tile_begin, int n_items) {
    for (int i = threadIdx.x; i <= n_items; i += 256) tb[i] = tile_begin[i];
    __syncthreads();
}

// (2) tile t -> the last item whose first tile is <= t, by bisection of the prefix array; everything block-uniform
struct WalkTile { int index; AdamItem it; int tl; };        // the item's index, the item, the tile's number inside it
__device__ __forceinline__ WalkTile walk_tile(const int* tb, const AdamItem* __restrict__ items, int n_items, int t) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return {lo, items[lo], t - tb[lo]};
}

// (3) where a lane's pieces lie.  A 1-D item (rows == 0) is a run of `cols` elements in tiles of 4,096: piece q of lane tid starts at
// element walk_run_index(tl, q).  A matrix tile is 64 x 64 at (r0, c0): lane tid owns columns gc .. gc + 3 of rows r0 + lr + 16 i.
__device__ __forceinline__ long long walk_run_index(int tl, int q) { return (long long)tl * 4096 + q * 1024 + (int)threadIdx.x * 4; }
__device__ __forceinline__ int walk_left(long long left) { return left >= 4 ? 4 : left > 0 ? (int)left : 0; }      // -> a piece's n
struct WalkGeom {
    int rows, cols, ldd, ldt;            // ldd, ldt: the leading dimensions of the W and W^T shadows (multiples of 8)
    int r0, c0, lr, c, gc;
    bool vec;                            // cols % 4 == 0: every 4-column group is whole and 16-byte aligned
};
__device__ __forceinline__ WalkGeom walk_geom(const AdamItem& it, int tl) {
    WalkGeom w;
    w.rows = it.rows; w.cols = it.cols; w.ldd = (it.cols + 7) & ~7; w.ldt = (it.rows + 7) & ~7;
    w.r0 = (tl / it.tiles_c) << 6; w.c0 = (tl % it.tiles_c) << 6;
    w.lr = (int)threadIdx.x >> 4; w.c = 4 * ((int)threadIdx.x & 15); w.gc = w.c0 + w.c;
    w.vec = (it.cols & 3) == 0;
    return w;
}

// Persistent 1-D grid of 256-thread workgroups over tiles [tile_first, total_tiles) of items[0, n_items).  1-D items: the pieces inside
// `cols` go to the Op and nothing else happens (whether `cols` reaches into the pad behind the tensor is the item table's business:
// the Adam items' runs do - Adam rewrites the pad - SAM's stop at the tensor's last element).  RUN_BATCH: all four loads of a run before
// the first finish, or piece by piece - the caller's choice.  Matrix tiles: all four loads, then per piece finish and - THE writer of the
// shadows - the new values into the LDS tile (zeros outside the matrix: the W^T shadow's pad rows read them), the W row store (8 packed
// bytes, or element by element), a barrier, the W^T store (8 consecutive source rows of one column per lane = 16 bytes of a W^T row),
// a barrier.  NT_SH: the shadow stores' cache hint.
template <bool NT_SH, bool RUN_BATCH, class Op>
__device__ __forceinline__ void walk_tiles(const AdamItem* __restrict__ items, const int* __restrict__ tile_begin, int n_items,
                                           int tile_first, int total_tiles, uint16_t* __restrict__ sh, Op& op) {
    __shared__ float tile[64][65];
    __shared__ int tb[M2F_ADAM_MAX_ITEMS + 1];
    const int tid = threadIdx.x;
    walk_prefix(tb, tile_begin, n_items);
    for (int t = tile_first + (int)blockIdx.x; t < total_tiles; t += gridDim.x) {
        const WalkTile wt = walk_tile(tb, items, n_items, t);
        const AdamItem& it = wt.it;
        op.item(wt.index, it);
        if (it.rows == 0) {
            if constexpr (RUN_BATCH) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long idx = walk_run_index(wt.tl, q);
                    const int n = walk_left(it.cols - idx);
                    if (n) op.load(q, it.off + idx, n, n == 4);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long idx = walk_run_index(wt.tl, q);
                const int n = walk_left(it.cols - idx);
                if (n) {
                    if constexpr (!RUN_BATCH) op.load(q, it.off + idx, n, n == 4);
                    op.finish(q, it.off + idx, n, n == 4);
                }
            }
            continue;
        }
        const WalkGeom w = walk_geom(it, wt.tl);
        int n[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                               // all loads of the tile first, then the arithmetic
            const int gr = w.r0 + w.lr + 16 * i;
            n[i] = gr < w.rows ? walk_left(w.cols - w.gc) : 0;
            op.load(i, it.off + (long long)gr * w.cols + w.gc, n[i], w.vec);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = w.lr + 16 * i, gr = w.r0 + r;
            const f32x4 nw = op.finish(i, it.off + (long long)gr * w.cols + w.gc, n[i], w.vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[r][w.c + e] = e < n[i] ? nw[e] : 0.f;
            if (n[i]) {
                uint16_t* q = sh + it.soff + (long long)gr * w.ldd + w.gc;
                if (w.vec) {
                    param_store<NT_SH>(reinterpret_cast<u32x2*>(q), param_bf16x4(nw));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (e < n[i]) q[e] = m2f_bf16_bits(nw[e]);
                }
            }
        }
        __syncthreads();
        {
            const int r8 = tid & 7;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cc = (tid >> 3) + 32 * j;
                const int gcol = w.c0 + cc, gr0 = w.r0 + 8 * r8;
                if (gcol < w.cols && gr0 < w.ldt) {
                    uint16_t h[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) h[k] = m2f_bf16_bits(tile[8 * r8 + k][cc]);
                    u32x4 x;
                    x.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); x.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
                    x.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16); x.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
                    param_store<NT_SH>(reinterpret_cast<u32x4*>(sh + it.soff_t + (long long)gcol * w.ldt + gr0), x);      // soff_t, ldt: multiples of 8
                }
            }
        }
        __syncthreads();
    }
}

// ---- the slice walk (ops.h ParamSlice) --------------------------------------------------------------------------------------------------
// One slice: at most M2F_PARAM_SLICE consecutive elements of ONE tensor (pads belong to no slice), 16 bytes per lane and piece (tensor
// offsets are multiples of 64 elements: 16-byte aligned); the last 1-3 elements of a tensor whose size is no multiple of 4 come as a piece
// with n < 4, nothing behind them is touched.  BATCH: pieces whose loads are all issued before the first finish (1: piece by piece) - the
// caller's choice.
template <int BATCH, class Op>
__device__ __forceinline__ void walk_slice(const ParamSlice& sl, Op& op) {
    const int tid = threadIdx.x;
#pragma unroll(BATCH == 1 ? 2 : 1)
    for (int r = 0; r < M2F_PARAM_SLICE / (1024 * BATCH); ++r) {
        if constexpr (BATCH > 1) {
#pragma unroll
            for (int j = 0; j < BATCH; ++j) {
                const int e = ((r * BATCH + j) * 256 + tid) * 4, n = walk_left(sl.n - e);
                if (n) op.load(j, sl.off + e, n, n == 4);
            }
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int e = ((r * BATCH + j) * 256 + tid) * 4, n = walk_left(sl.n - e);
            if (n) {
                if constexpr (BATCH == 1) op.load(j, sl.off + e, n, n == 4);
                op.finish(j, sl.off + e, n, n == 4);
            }
        }
    }
}
