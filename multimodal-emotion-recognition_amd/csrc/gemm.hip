// Grouped MFMA GEMM for the M2FNet hot path (gfx950 / CDNA4, wave64).
//
//   C[M,N] = epilogue( sum_k A(m,k) * B(n,k) )      (see ops.h for layouts / epilogue order)
//
// Replaces every nn.Linear / in-projection / out-projection call the reference's model makes
// (reference src/model.py:14,18,111-113,123-125,143 and torch's TransformerEncoderLayer internals)
// in forward, input-gradient and weight-gradient form.
//
// Design (MI355X) - two kernel families sharing one C/D layout and one fused epilogue:
//   * F32 mode (the 1e-3 parity mode) and the fallback for operands without bf16 shadows: `m2f_gemm_kernel`, fp32-source.
//     One workgroup = 4 wavefronts (2x2), each owning (BM/2)x(BN/2) of the tile as 32x32 blocks of
//     v_mfma_f32_32x32x2_f32 (exact fp32, 157 TF peak) or, in BF16 mode, v_mfma_f32_32x32x16_bf16 with the operands
//     rounded to bf16 while being staged.  Register-staged operands (coalesced 16-byte loads one k-tile ahead), LDS images
//     laid out for conflict-free fragment reads ([k][row] floats with row stride BR+1 | [row][k] bf16 with 272-byte rows).
//   * BF16 mode proper: `m2f_gemm16_kernel` (+ `_dense_` variant), bf16-SOURCE: every operand also exists as a
//     bf16 shadow in HBM (half the bytes through the per-CU L1 fill path that bounds these GEMMs).  Workgroups of 8 waves
//     split into 4 producer waves (global -> register ring of D k-tiles -> LDS) and 4 consumer waves (LDS -> MFMA ->
//     epilogue); tiles 64x64 (chain launches), 128x128 or 256x128 (text encoder); see the comment above gemm16_body.
//     Chip-filling launches and the weight-gradient table launch (m2f_launch_gemm_table) run the LDS-DMA forms instead:
//     gemm_ring.h and gemm_p8.h.  Which form a launch takes is decided in gemm_dispatch.hip; this unit holds the register-staged
//     kernels and how they are launched (m2f_launch_gemm_staged).
//   * "grouped": one launch covers several independent problems (text+audio branch, q/k/v of a fusion layer, split
//     concat) so the 256 CUs see more workgroups per launch and the launch-latency-bound chain gets shorter;
//   * the epilogue fuses bias, ReLU / exact GELU, dropout, residual add, ReLU-gate and accumulate (32-bit offsets from
//     uniform bases, optional terms behind block-uniform branches) and writes the bf16 shadow of C; the row-contiguous
//     wgrad form also emits the bias gradient (column sums of dY) from the tiles it already streams.
#include "common.h"
#include "ops.h"
#include <type_traits>
#include <cstring>

// No floating-point contraction in this file: several kernels restate the same formulas in different surroundings (ring and
// register-staged GEMM epilogues, fp32 and bf16 attention forms, flat and shadow-writing Adam), and with -ffp-contract=fast (the
// HIP default) the compiler is free to fuse a*b+c in one of them and not in the other - a 1-ulp difference that would break the
// bit-for-bit comparisons the tests make between the forms.  These kernels are bound by memory or by MFMA, not by VALU multiplies.
#pragma clang fp contract(off)

// Experiment knobs (register sets in flight).  NOTE: builds that spill VGPRs are NOT safe with the inline-asm staging
// loads (see Stage16KC::wait_loaded): D = 3 of the 128-VGPR chain build spills and faults.
#ifndef M2F_CHAIN_D
#define M2F_CHAIN_D 2         // register sets in flight of the 64x64 chain build (experiment knob)
#endif

namespace {

// ---------------------------------------------------------------------------------------------------------
// Operand staging: global (fp32) -> registers -> LDS image.
//   KC operand: element (row, k) at p[row*ld + k];  RC operand: element (row, k) at p[k*ld + row].
// The staging code is the instruction-issue bottleneck of these small-M GEMMs (measured: ~2 us per k-tile when
// every element carried its own bounds test and 64-bit address), so:
//   * per-thread element offsets are computed ONCE per workgroup (rows clamped into range, 32-bit), a k-tile only
//     adds a wave-uniform base;
//   * interior tiles (the common case, wave-uniform test) take a path with no masking at all; only edge tiles pay
//     for per-element predicates;
//   * every global load is unconditional (edge lanes read a clamped in-range address and are zeroed at store time):
//     hipcc turns a guarded load into a branch + s_waitcnt vmcnt(0) per load, which serialises the tile fetch
//     (cdna_hip_programming.md, ".s-level traps" (c));
//   * nothing consumes a loaded value before store(), so both operands' loads of a k-tile stay in flight while
//     earlier tiles are multiplied.
// ---------------------------------------------------------------------------------------------------------
template <int PREC, bool RC, int BR, int BK_, bool VEC>
struct Stage {
    static constexpr int BK = BK_;
    static constexpr bool F32 = (PREC == M2F_PREC_F32);
    // floats per task: F32 4 (one float4) | BF16-KC 8 (8 consecutive k) | BF16-RC 32 (8 k x 4 rows patch)
    static constexpr int FPT = F32 ? 4 : (RC ? 32 : 8);
    static constexpr int NT = BR * BK / FPT / 256;                       // staging tasks per thread
    static_assert(NT >= 1 && (BR * BK) % (FPT * 256) == 0, "tile must split evenly over 256 threads");
    static constexpr int KCH = BK / (F32 ? 4 : 8);                       // KC: chunks along k per row
    static constexpr int LDR = BR + 1;                                   // F32 LDS row stride (floats), image [k][row]
    static constexpr int ROWB = BK * 2 + 16;                             // BF16 LDS row stride (bytes), image [row][k]
    static constexpr int LDS_BYTES = F32 ? BK * LDR * 4 : BR * ROWB;

    float v[NT][FPT];
    int off[NT];             // element offset of task t at kbase = 0 (row clamped into range)
    int ld_;                 // leading dimension of the current segment
    int rows_, row0_, kseg_, kbase_;
    bool full_;              // tile in flight needs no masking (wave-uniform)
    int seg_ = -1;           // operand segment the offsets were set up for

    // task decomposition (t-th task of this thread)
    __device__ __forceinline__ static void task_rc(int id, int& r, int& k) {
        if constexpr (!RC) { r = id / KCH; k = (F32 ? 4 : 8) * (id % KCH); }           // KC: row r, k offset
        else if constexpr (F32) { constexpr int CH = BR / 4; k = id / CH; r = 4 * (id % CH); }   // float4 along rows
        else { constexpr int CH = BR / 4; k = 8 * (id / CH); r = 4 * (id % CH); }       // 8 k x 4 rows patch
    }

    __device__ __forceinline__ void setup(int ld, int rows, int row0, int tid) {
        ld_ = ld; rows_ = rows; row0_ = row0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int r, k;
            task_rc(tid + 256 * t, r, k);
            int gr = row0 + r;
            // clamp so that every (vector) load stays inside the operand; clamped lanes are masked at store time
            const int last = VEC && RC ? rows - 4 : rows - 1;
            gr = gr < last ? gr : (last > 0 ? last : 0);
            off[t] = RC ? k * ld + gr : gr * ld + k;
        }
    }

    template <bool FULL>
    __device__ __forceinline__ void issue_impl(const float* __restrict__ pt) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int r, k;
            task_rc(threadIdx.x + 256 * t, r, k);
            if constexpr (!RC) {
                constexpr int NV = FPT / 4;
#pragma unroll
                for (int h = 0; h < NV; ++h) {
                    if constexpr (VEC) {
                        int o = off[t] + 4 * h;
                        if constexpr (!FULL) o = (kbase_ + k + 4 * h < kseg_) ? o : off[t] - k - kbase_;   // row start (k = 0)
                        const f32x4 x = *reinterpret_cast<const f32x4*>(pt + o);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[t][4 * h + e] = x[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            int o = off[t] + 4 * h + e;
                            if constexpr (!FULL) o = (kbase_ + k + 4 * h + e < kseg_) ? o : off[t] - k - kbase_;
                            v[t][4 * h + e] = pt[o];
                        }
                    }
                }
            } else {
                constexpr int NK = F32 ? 1 : 8;                       // k rows of the patch
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    int o = off[t] + j * ld_;
                    if constexpr (!FULL) o = (kbase_ + k + j < kseg_) ? o : off[t] - (k + kbase_) * ld_;    // k = 0 row
                    if constexpr (VEC) {
                        const f32x4 x = *reinterpret_cast<const f32x4*>(pt + o);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[t][4 * j + e] = x[e];
                    } else {
                        // scalar path: clamp each element's row separately (off[] holds the clamped first row)
                        int grc = row0_ + r;
                        grc = grc < rows_ - 1 ? grc : rows_ - 1;
                        const int room = rows_ - 1 - grc;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[t][4 * j + e] = pt[o + (e < room ? e : room)];
                    }
                }
            }
        }
    }

    // Issue the loads of the tile at (kbase) of segment pointer p.  kseg = 0 marks a tile past the end (all masked).
    __device__ __forceinline__ void issue(const float* __restrict__ p, int kseg, int kbase) {
        kseg_ = kseg; kbase_ = kbase;
        full_ = (row0_ + BR <= rows_) && (kbase + BK <= kseg);
        const float* pt = p + (RC ? (size_t)kbase * ld_ : (size_t)kbase);
        if (full_) issue_impl<true>(pt);
        else issue_impl<false>(pt);
    }

    __device__ __forceinline__ bool elem_ok(int r, int k) const { return row0_ + r < rows_ && kbase_ + k < kseg_; }

    // Mask (edge tiles only), optional ReLU, optional column sums (wgrad bias gradient), convert, write LDS.
    template <bool FULL>
    __device__ __forceinline__ void store_impl(char* lds, bool relu, bool do_cs, f32x4& cs) {
        if constexpr (!FULL) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                int r, k;
                task_rc(threadIdx.x + 256 * t, r, k);
#pragma unroll
                for (int e = 0; e < FPT; ++e) {
                    bool ok;
                    if constexpr (!RC) ok = elem_ok(r, k + e);
                    else ok = elem_ok(r + (e & 3), k + (e >> 2));
                    v[t][e] = ok ? v[t][e] : 0.f;
                }
            }
        }
        if (relu) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < FPT; ++e) v[t][e] = fmaxf(v[t][e], 0.f);
        }
        if constexpr (RC) {
            if (do_cs) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < FPT; ++e) cs[e & 3] += v[t][e];
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int r, k;
            task_rc(threadIdx.x + 256 * t, r, k);
            if constexpr (F32 && !RC) {
                float* f = reinterpret_cast<float*>(lds);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[(k + e) * LDR + r] = v[t][e];
            } else if constexpr (F32 && RC) {
                float* f = reinterpret_cast<float*>(lds);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[k * LDR + r + e] = v[t][e];
            } else if constexpr (!RC) {
                bf16x8 h;
#pragma unroll
                for (int e = 0; e < 8; ++e) h[e] = (__bf16)v[t][e];
                *reinterpret_cast<bf16x8*>(lds + r * ROWB + k * 2) = h;
            } else {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {                     // transpose the 8k x 4rows patch: one b128 per row
                    bf16x8 h;
#pragma unroll
                    for (int j = 0; j < 8; ++j) h[j] = (__bf16)v[t][4 * j + rr];
                    *reinterpret_cast<bf16x8*>(lds + (r + rr) * ROWB + k * 2) = h;
                }
            }
        }
    }
    __device__ __forceinline__ void store(char* lds, bool relu, bool do_cs, f32x4& cs) {
        if (full_) store_impl<true>(lds, relu, do_cs, cs);
        else store_impl<false>(lds, relu, do_cs, cs);
    }
};


// Fused epilogue shared by the fp32-source and bf16-source kernels:
//   +bias[n] -> relu -> dropout(site) -> +res[m,n] -> *(gate[m,n] > 0 ? gate_scale : 0) -> (C += | C =) [-> bf16 shadow of C]
// Side loads are unconditional (clamped) and issued before the arithmetic; stores are predicated.
// GELU is a COMPILE-TIME variant: carrying the erf expansion (and its constants) in every instantiation doubled the SGPR
// spills of the chain kernels (24 -> 52) and cost the M2FNet step 3.4 %; only the text encoder's GEMMs use it.
// (m2f_gelu: common.h)
template <int MI, int NI, int BM, int BN, bool GELU = false, bool SCALE = false, bool GELU_POLY = false>
__device__ __forceinline__ void gemm_epilogue(const GemmBatch& gb, const GemmProblem& P, f32x16 (&acc)[MI][NI], int m0, int n0,
                                              int lane, int wm, int wn) {
    const int M = P.M, N = P.N;
    const uint32_t flags = P.flags;
    const float* __restrict__ bias = P.bias;
    const char* __restrict__ res = reinterpret_cast<const char*>(P.res);
    const char* __restrict__ gate = reinterpret_cast<const char*>(P.gate);
    char* __restrict__ C = reinterpret_cast<char*>(P.c);
    char* __restrict__ C16 = reinterpret_cast<char*>(m2f_shadow_of(gb.sh, P.c));
    const int ldc = P.ldc, ldres = P.ldres, ldgate = P.ldgate;
    const float gscale = P.gate_scale;
    const bool relu_out = flags & GF_RELU_OUT, accum = flags & GF_ACCUM;
    const uint32_t site = P.drop_site;
    uint32_t key = 0;
    if (site) key = m2f_site_key(gb.rng, site);
    // Everything below is indexed with 32-bit element offsets from the (uniform) base pointers - the saddr form of
    // global_load / global_store - and every optional term sits behind ONE block-uniform branch per 32x32 block: the
    // per-element 64-bit multiplies and branches of the first version cost 2 us (64x64 tile) to 7 us (128x128) per
    // workgroup, more than the k-loop of these small-K problems.
    const bool interior = (m0 + BM <= M) && (n0 + BN <= N);         // block-uniform: no clamping / predicates needed
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int col = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
            const bool col_ok = col < N;
            const int colc = col_ok ? col : N - 1;
            const int row_base = m0 + wm * (BM / 2) + i * 32 + 4 * (lane >> 5);
            const float bv = bias ? bias[colc] : 0.f;
            // row of element r: row_base + (r & 3) + 8 * (r >> 2)
            uint32_t oc[16], orr[16], og[16];
            bool ok[16];
            if (interior) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = (r & 3) + 8 * (r >> 2);
                    oc[r] = (uint32_t)((row_base + dr) * ldc + col);
                    ok[r] = true;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row_base + (r & 3) + 8 * (r >> 2);
                    const int rowc = row < M ? row : M - 1;
                    oc[r] = (uint32_t)(rowc * ldc + colc);
                    ok[r] = row < M && col_ok;
                }
            }
            float rv[16], gv[16], cv[16];
            if (res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row_base + (r & 3) + 8 * (r >> 2);
                    orr[r] = (uint32_t)((interior ? row : (row < M ? row : M - 1)) * ldres + colc);
                    rv[r] = *reinterpret_cast<const float*>(res + (size_t)(orr[r] * 4u));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = 0.f;
            }
            if (gate) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row_base + (r & 3) + 8 * (r >> 2);
                    og[r] = (uint32_t)((interior ? row : (row < M ? row : M - 1)) * ldgate + colc);
                    gv[r] = *reinterpret_cast<const float*>(gate + (size_t)(og[r] * 4u));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) gv[r] = 1.f;
            }
            if (accum) {
#pragma unroll
                for (int r = 0; r < 16; ++r) cv[r] = *reinterpret_cast<const float*>(C + (size_t)(oc[r] * 4u));
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) cv[r] = 0.f;
            }
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x = (SCALE ? acc[i][j][r] * P.acc_scale : acc[i][j][r]) + bv;
                if (relu_out) x = fmaxf(x, 0.f);
                v[r] = x;
            }
            if constexpr (GELU) {
                if (flags & GF_GELU_OUT) {                      // block-uniform
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = m2f_gelu<GELU_POLY>(v[r]);
                }
            }
            if (site) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row_base + (r & 3) + 8 * (r >> 2);
                    v[r] = m2f_keep(key, (uint32_t)row * (uint32_t)N + (uint32_t)col, gb.drop_thresh) ? v[r] * gb.drop_scale : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x = v[r] + rv[r];
                if (gate) x = gv[r] > 0.f ? x * gscale : 0.f;
                v[r] = x + cv[r];
            }
            if constexpr (SCALE) {
                if (P.c8) {                                     // block-uniform: e4m3 result instead of fp32 C
                    const float s8 = P.c8_scale;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (ok[r]) P.c8[oc[r]] = (uint8_t)(m2f_fp8x4_bits(v[r] * s8, 0.f, 0.f, 0.f) & 0xFFu);
                    continue;
                }
            }
            if (interior) {
#pragma unroll
                for (int r = 0; r < 16; ++r) *reinterpret_cast<float*>(C + (size_t)(oc[r] * 4u)) = v[r];
                if (C16) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) *reinterpret_cast<uint16_t*>(C16 + (size_t)(oc[r] * 2u)) = m2f_bf16_bits(v[r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (ok[r]) {
                        *reinterpret_cast<float*>(C + (size_t)(oc[r] * 4u)) = v[r];
                        if (C16) *reinterpret_cast<uint16_t*>(C16 + (size_t)(oc[r] * 2u)) = m2f_bf16_bits(v[r]);
                    }
            }
        }
    }
}

// XCD-aware block order.  Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8, each with its own
// L2), so consecutive blocks never share an L2.  Remap b -> pos so that every XCD walks a CONTIGUOUS range of the
// launch's tile list, and order tiles with the M index fastest: an XCD then owns whole column panels of B (the weight,
// cold in HBM), which are fetched into one L2 once instead of into all eight.  Bijective for any grid size; a different
// hardware placement only changes speed, never results.
__device__ __forceinline__ int xcd_remap(int b, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, x = b & 7, j = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

// LDS-only workgroup barrier: wait for this wave's LDS traffic, then s_barrier.  __syncthreads() carries a
// workgroup-scope fence for which hipcc also drains vmcnt(0), i.e. the prefetched global loads of the next
// k-tiles - exactly the loads that must stay in flight across the barrier.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int PREC, bool A_RC, bool B_RC, int BM, int BN, int BK, bool VEC, bool GELU = false>
__global__ __launch_bounds__(256) void m2f_gemm_kernel(const GemmBatch gb) {
    using SA = Stage<PREC, A_RC, BM, BK, VEC>;
    using SB = Stage<PREC, B_RC, BN, BK, VEC>;
    constexpr int MI = BM / 64, NI = BN / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    int pi = 0;
#pragma unroll
    for (int i = 1; i < M2F_GEMM_MAX_PROBLEMS; ++i)
        if (i < gb.count && (int)blockIdx.x >= gb.pr[i].tile_begin) pi = i;
    const GemmProblem& P = gb.pr[pi];

    const int M = P.M, N = P.N;
    // split-K: `splitk` consecutive workgroups share one output tile, each reduces a slice of the k-tile list
    const int S = P.splitk;
    const int tb = (int)blockIdx.x - P.tile_begin;
    const int tl = tb / S, slice = tb - tl * S;
    const int m0 = (tl / P.tiles_n) * BM, n0 = (tl % P.tiles_n) * BN;
    const uint32_t flags = P.flags;
    const bool reluA = flags & GF_RELU_A, reluB = flags & GF_RELU_B;
    const int k0 = P.a.k[0], k1 = P.a.k[1];
    const int nk0 = (k0 + BK - 1) / BK, nk_all = nk0 + (k1 + BK - 1) / BK;
    const int kt_begin = (slice * nk_all) / S, nk = ((slice + 1) * nk_all) / S - kt_begin;   // this slice: nk k-tiles

    char* ldsA = smem;
    char* ldsB = smem + 2 * SA::LDS_BYTES;

    // Two register sets: the global loads of k-tile t+2 / t+3 are in flight while tile t is multiplied, so a
    // workgroup keeps ~2 tiles of HBM/L2 traffic outstanding (these GEMMs are latency-bound, M = B*L is small).
    SA sa0, sa1;
    SB sb0, sb1;
    f32x4 colsum = {0.f, 0.f, 0.f, 0.f}, cs_unused = {0.f, 0.f, 0.f, 0.f};
    const bool want_bg = A_RC && P.bias_grad != nullptr && n0 == 0;

    // UNCONDITIONAL: a k-tile index past the end issues the same number of loads (all masked to zero at store
    // time).  A branch around the prefetch would make the number of loads in flight path-dependent, and hipcc then
    // drains vmcnt to 0 at every store phase (seen in the .s) - no overlap left.
    auto load_tile = [&](SA& sa, SB& sb, int kt_raw) {
        const bool tv = kt_raw < nk;
        const int kt = tv ? kt_begin + kt_raw : 0;
        const int seg = kt >= nk0 ? 1 : 0;
        const int kbase = (seg ? kt - nk0 : kt) * BK;
        if (sa.seg_ != seg) {                                  // wave-uniform, at most twice per workgroup
            sa.setup(P.a.ld[seg], M, m0, tid); sa.seg_ = seg;
            sb.setup(P.b.ld[seg], N, n0, tid); sb.seg_ = seg;
        }
        sa.issue(P.a.p[seg], tv ? P.a.k[seg] : 0, kbase);
        sb.issue(P.b.p[seg], tv ? P.b.k[seg] : 0, kbase);
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int cur) {
        const char* a_l = ldsA + cur * SA::LDS_BYTES;
        const char* b_l = ldsB + cur * SB::LDS_BYTES;
        if constexpr (PREC == M2F_PREC_F32) {
            const float* af = reinterpret_cast<const float*>(a_l) + wm * (BM / 2) + (lane & 31);
            const float* bf = reinterpret_cast<const float*>(b_l) + wn * (BN / 2) + (lane & 31);
#pragma unroll 4
            for (int ks = 0; ks < BK / 2; ++ks) {
                const int kk = 2 * ks + (lane >> 5);
                float a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = af[kk * SA::LDR + i * 32];
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = bf[kk * SB::LDR + j * 32];
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        } else {
            const char* ab = a_l + (wm * (BM / 2) + (lane & 31)) * SA::ROWB + (lane >> 5) * 16;
            const char* bb = b_l + (wn * (BN / 2) + (lane & 31)) * SB::ROWB + (lane >> 5) * 16;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                bf16x8 a[MI], b[NI];
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(ab + i * 32 * SA::ROWB + ks * 32);
#pragma unroll
                for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const bf16x8*>(bb + j * 32 * SB::ROWB + ks * 32);
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
    };

    load_tile(sa0, sb0, 0);
    load_tile(sa1, sb1, 1);
    sa0.store(ldsA, reluA, want_bg, colsum);
    sb0.store(ldsB, reluB, false, cs_unused);
    lds_barrier();
    load_tile(sa0, sb0, 2);

    for (int kt = 0; kt < nk; kt += 2) {
        // even phase: multiply tile kt (buffer 0); stage tile kt+1 (register set 1) into buffer 1
        compute(0);
        // (stores are unconditional too: past the last tile they write the all-zero masked tile to an unused buffer)
        sa1.store(ldsA + SA::LDS_BYTES, reluA, want_bg, colsum);
        sb1.store(ldsB + SB::LDS_BYTES, reluB, false, cs_unused);
        lds_barrier();
        load_tile(sa1, sb1, kt + 3);
        if (kt + 1 >= nk) break;
        // odd phase: multiply tile kt+1 (buffer 1); stage tile kt+2 (register set 0) into buffer 0
        compute(1);
        sa0.store(ldsA, reluA, want_bg, colsum);
        sb0.store(ldsB, reluB, false, cs_unused);
        lds_barrier();
        load_tile(sa0, sb0, kt + 4);
    }

    // ---- wgrad: bias gradient = column sums of the A operand (dY) over the reduction dim ----------
    if constexpr (A_RC) {
        if (want_bg) {      // block-uniform
            float* red = reinterpret_cast<float*>(smem);
            constexpr int CH = BM / 4, G = 256 / CH;       // thread = (k-group g, 4 rows 4*rc..): same rows for all its tasks
            const int g = tid / CH, rc = tid % CH;
#pragma unroll
            for (int e = 0; e < 4; ++e) red[g * BM + 4 * rc + e] = colsum[e];
            __syncthreads();
            if (tid < BM) {
                float sum = 0.f;
                for (int q = 0; q < G; ++q) sum += red[q * BM + tid];
                // (GF_ACCUM, the accumulate form of a weight gradient: the bias gradient accumulates with C - old + new, as C does)
                if (m0 + tid < M) P.bias_grad[m0 + tid] = (P.flags & GF_ACCUM) ? P.bias_grad[m0 + tid] + sum : sum;
            }
        }
    }

    // ---- split-K: publish the partial tile; the LAST arriving slice sums all partials (fixed order -> bitwise
    // reproducible) and runs the epilogue.  Agent-scope release/acquire around a relaxed ticket, valid for any
    // placement of the slices over CUs / XCDs (cdna_hip_programming.md, "In-launch split-K reduction").
    if (S > 1) {
        static_assert(MI * NI * 16 * 256 == BM * BN, "slab layout");
        float* slab = gb.splitk_ws + (size_t)(P.slab_begin + tl * S) * (BM * BN);
        float* mine = slab + (size_t)slice * (BM * BN);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[((i * NI + j) * 16 + r) * 256 + tid] = acc[i][j][r];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem);
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned t = __hip_atomic_fetch_add(gb.splitk_cnt + P.cnt_begin + tl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = (t == (unsigned)(S - 1)) ? 1 : 0;
        }
        __syncthreads();
        if (*flag == 0) return;                              // block-uniform
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(gb.splitk_cnt + P.cnt_begin + tl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-arm
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float sum = 0.f;
                    for (int q = 0; q < S; ++q) sum += slab[(size_t)q * (BM * BN) + ((i * NI + j) * 16 + r) * 256 + tid];
                    acc[i][j][r] = sum;
                }
    }

    gemm_epilogue<MI, NI, BM, BN, GELU>(gb, P, acc, m0, n0, lane, wm, wn);
}

// =========================================================================================================
// bf16-SOURCE kernel (bf16 mode): operands are read from the bf16 shadows (half the bytes through the per-CU load
// pipe, which is what bounds these GEMMs), 16 bytes = 8 elements per load, no conversion, D k-tiles in flight.
// Pad columns of every shadow are zero, so a logical width that is not a multiple of 8 needs no element masks.
// =========================================================================================================
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {
    const uint32_t m = ((v >> 15) & 0x00010001u) * 0xFFFFu;      // 0xFFFF in every half whose sign bit is set
    return v & ~m;
}
__device__ __forceinline__ float bf16lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf16hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xFFFF0000u); }

// 16-byte load through an explicitly GLOBAL pointer (a native vector type: HIP's uint4 is a class whose copy goes through a
// generic reference and loses the address space again)
typedef unsigned int m2f_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld16_global(const void* p) {
    const m2f_u32x4 r = *(const __attribute__((address_space(1))) m2f_u32x4*)p;
    return make_uint4(r.x, r.y, r.z, r.w);
}

template <int BR, int BK>
struct Stage16KC {                       // element (row, k) at q[row*ld + k]
    static constexpr int KCH = BK / 8, NT = BR * KCH / 256;
    static constexpr int ROWB = BK * 2 + 16, LDS_BYTES = BR * ROWB;
    static_assert(NT >= 1 && (BR * KCH) % 256 == 0, "tile split");
    m2f_u32x4 v[NT];
    uint32_t off[NT];                    // BYTE offset of chunk t from the row-panel base at kbase = 0 (row clamped)
    int rows_, row0_, kpad_, kbase_, tid_;
    bool full_;
    __device__ __forceinline__ void setup(int ld, int rows, int row0, int tid) {
        rows_ = rows; row0_ = row0; tid_ = tid;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int id = tid + 256 * t, r = id / KCH, kc = id % KCH;
            int gr = row0 + r;
            gr = gr < rows - 1 ? gr : rows - 1;
            off[t] = 2u * (uint32_t)(gr * ld + 8 * kc);
        }
    }
    // uniform 64-bit base + zero-extended 32-bit lane offset: the saddr form of global_load (no per-load 64-bit VALU add)
    // The address-space cast matters wherever the compiler cannot prove an operand pointer global (one read from device
    // memory): it then emits FLAT loads - which also count on lgkmcnt, share ordering with the ds_writes and turn every
    // counted wait of the ring into vmcnt(0) lgkmcnt(0).
    __device__ __forceinline__ static m2f_u32x4 ld16(const char* base, uint32_t o) {
        return *(const __attribute__((address_space(1))) m2f_u32x4*)(base + (size_t)o);
    }
    template <bool ASM = false>
    __device__ __forceinline__ void issue(const uint16_t* __restrict__ q, int kseg, int kbase) {
        kpad_ = (kseg + 7) & ~7; kbase_ = kbase;
        full_ = (row0_ + BR <= rows_) && (kbase + BK <= kpad_);
        const char* pt = reinterpret_cast<const char*>(q + kbase);
        // ONE straight-line path for interior and edge tiles (selects, no branch): with the loads of a set split over two
        // branches the waitcnt pass loses count at the merge and every wait of the ring becomes vmcnt(0)
        static_assert(256 % KCH == 0, "chunk column is the same for every t");
        const int kc = tid_ % KCH;
        const uint32_t back = (kbase + 8 * kc < kpad_) ? 0u : 16u * kc;     // past the padded width: this tile's first chunk
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            uint32_t o = off[t] - back;
            o = kseg == 0 ? 0u : o;               // dead tile past the end of the k-loop: every lane reads the same 16 bytes
            if constexpr (ASM) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v[t]) : "v"(o), "s"(pt) : "memory");
            else v[t] = ld16(pt, o);
        }
    }
    // ASM issue: the compiler does not know these registers are in flight, so the caller waits by hand - `newer` = loads
    // issued after the last one of this set.  The registers are tied through the statement so that no use can be scheduled
    // above it.
    template <int NEWER>
    __device__ __forceinline__ void wait_loaded() {
        static_assert(NEWER >= 0 && NEWER <= 63 && NT <= 16, "vmcnt immediate / operand count");
        if constexpr (NT == 1) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v[0]) : "n"(NEWER) : "memory");
        else if constexpr (NT == 2) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(v[0]), "+v"(v[1]) : "n"(NEWER) : "memory");
        else if constexpr (NT == 4)
            asm volatile("s_waitcnt vmcnt(%4)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "n"(NEWER) : "memory");
        else if constexpr (NT == 8)
            asm volatile("s_waitcnt vmcnt(%8)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]),
                         "+v"(v[7]) : "n"(NEWER) : "memory");
        else static_assert(NT == 1 || NT == 2 || NT == 4 || NT == 8, "chunks per thread");
    }
    __device__ __forceinline__ void store(char* lds, bool relu) {
        // the rare fix-ups (edge masks, relu of the operand) sit behind ONE block-uniform branch, so the common path
        // is eight back-to-back ds_write_b128 with progressive vmcnt waits and no control flow in between
        if (!full_ || relu) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int id = tid_ + 256 * t, r = id / KCH, kc = id % KCH;
                m2f_u32x4 x = v[t];
                const bool ok = full_ || ((row0_ + r < rows_) && (kbase_ + 8 * kc < kpad_));
                if (!ok) x = (m2f_u32x4){0u, 0u, 0u, 0u};
                if (relu) { x.x = relu_bf16x2(x.x); x.y = relu_bf16x2(x.y); x.z = relu_bf16x2(x.z); x.w = relu_bf16x2(x.w); }
                v[t] = x;
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int id = tid_ + 256 * t, r = id / KCH, kc = id % KCH;
            *reinterpret_cast<m2f_u32x4*>(lds + r * ROWB + kc * 16) = v[t];
        }
    }
};

template <int BR, int BK>
struct Stage16RC {   // element (row, k) at q[k*ld + row]; one 8(k) x 8(row) patch per active thread
    // LDS image is K-MAJOR: [k][row] bf16 with row stride ROWK = 2*BR + 64 bytes, written exactly as loaded (16-byte
    // vectors, lanes = consecutive row groups -> conflict-free) and consumed with ds_read_b64_tr_b16, the gfx950
    // transposing LDS read (4 k-rows x 16 rows per 16-lane group; with this stride the 4 k-rows of a group fall on
    // disjoint bank ranges).  No register transposes, no scattered stores.
    static constexpr int KP = BK / 8, RP = BR / 8, NPATCH = KP * RP;
    static constexpr int ROWK = 2 * BR + 16, LDS_BYTES = BK * ROWK;   // +16: 2-way conflicts on the tr reads, but 2 workgroups fit a CU
    uint4 v[8];
    int off, kp_, rp_;
    int ld_, rows_, row0_, kseg_, kbase_;
    bool full_, active_;
    __device__ __forceinline__ void setup(int ld, int rows, int row0, int pid) {
        static_assert(NPATCH == 128, "one patch per thread of a 128-thread half");
        ld_ = ld; rows_ = rows; row0_ = row0;
        active_ = pid >= 0 && pid < NPATCH;
        const int p = active_ ? pid : 0;
        kp_ = p / RP; rp_ = p % RP;
        const int rpad = (rows + 7) & ~7;
        int gr = row0 + 8 * rp_;
        gr = gr < rpad - 8 ? gr : rpad - 8;
        off = 8 * kp_ * ld + (gr > 0 ? gr : 0);
    }
    __device__ __forceinline__ void issue(const uint16_t* __restrict__ q, int kseg, int kbase) {
        kseg_ = kseg; kbase_ = kbase;
        full_ = (row0_ + BR <= rows_) && (kbase + BK <= kseg);
        if (!active_) return;                                   // wave-uniform (patches are dealt per 128-thread half)
        const uint16_t* pt = q + (size_t)kbase * ld_;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int o = off + j * ld_;
            if (!full_) o = (kbase + 8 * kp_ + j < kseg) ? o : off - 8 * kp_ * ld_ - kbase * ld_;   // else: k = 0 row
            if (kseg == 0) o = 0;                 // dead tile past the end of the k-loop: one broadcast line
            v[j] = ld16_global(pt + o);
        }
    }
    __device__ __forceinline__ void store(char* lds, bool relu, bool do_cs, float (&cs)[8]) {
        if (!active_) return;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            if (!full_) {
                const bool kok = kbase_ + 8 * kp_ + j < kseg_;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int r = row0_ + 8 * rp_ + 2 * m;
                    uint32_t keep = 0u;
                    if (kok && r < rows_) keep |= 0x0000FFFFu;
                    if (kok && r + 1 < rows_) keep |= 0xFFFF0000u;
                    w[m] &= keep;
                }
            }
            if (relu) {
#pragma unroll
                for (int m = 0; m < 4; ++m) w[m] = relu_bf16x2(w[m]);
            }
            if (do_cs) {
#pragma unroll
                for (int m = 0; m < 4; ++m) { cs[2 * m] += bf16lo(w[m]); cs[2 * m + 1] += bf16hi(w[m]); }
            }
            *reinterpret_cast<uint4*>(lds + (8 * kp_ + j) * ROWK + 16 * rp_) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
};

typedef short m2f_s16x4 __attribute__((ext_vector_type(4)));
// MFMA 32x32x16 operand fragment (8 consecutive k of row `row`) out of a K-major LDS image via two transposing reads.
// Per 16-lane group g: lane 4q+p supplies the address of k-row (4t + q), rows 4p..4p+3; lane i receives row i.
__device__ __forceinline__ bf16x8 frag_from_kmajor(const char* img, int rowk, int row_base32, int k0, int lane) {
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const int kq = k0 + 8 * (g >> 1) + q;                       // + 4t
    const int col = row_base32 + 16 * (g & 1) + 4 * p;
    const char* a0 = img + kq * rowk + col * 2;
    const m2f_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (m2f_s16x4 __attribute__((address_space(3)))*)(const_cast<char*>(a0)));
    const m2f_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (m2f_s16x4 __attribute__((address_space(3)))*)(const_cast<char*>(a0 + 4 * rowk)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, r);
}

// Workgroup = 8 waves in two ROLES (wave-specialised): waves 0-3 are CONSUMERS (LDS fragments -> MFMA -> epilogue,
// 2x2 over the tile), waves 4-7 are PRODUCERS (global -> registers, D k-tiles in flight -> LDS image).  With one
// workgroup per CU - all these small-M launches offer - a SIMD then holds one wave of each role, so the address
// arithmetic / ds_write stream of tile k+1 issues in the shadow of the ds_read + MFMA run of tile k instead of in front
// of it (measured before the split: 0.62 us per 128-wide k-tile, ~40 % of it instruction issue of one wave per SIMD,
// MFMA busy 13 %).  The two roles run separate loops with the same barrier count, so their register sets (the load ring
// vs accumulators + fragments) overlap in the allocation instead of adding up.
#ifdef M2F_EXP_TIMING
__device__ unsigned long long m2f_dbg[64];
#define M2F_TS(slot) do { if (blockIdx.x == 0 && (threadIdx.x & 255) == 0) m2f_dbg[(slot) + (threadIdx.x >= 256 ? 16 : 0)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define M2F_TS(slot) do {} while (0)
#endif
// FP8: the operands are OCP e4m3 bytes.  The producers are unchanged - a k-tile is BK byte PAIRS per row either way (the
// launcher passes k and ldq in byte pairs) - only the consumers differ: 2*BK/16 slices of v_mfma_f32_32x32x16_fp8_fp8 with
// 8-byte fragments, and the epilogue de-quantises the accumulator.
template <bool A_RC, bool B_RC, int BM, int BN, int BK, int D, bool GELU = false, bool FP8 = false>
__device__ __forceinline__ void gemm16_body(const GemmBatch& gb) {
    static_assert(!(A_RC && !B_RC), "layouts: NT, NN, TN");
    static_assert(!FP8 || (!A_RC && !B_RC), "fp8: forward form only");
    constexpr bool TN = A_RC && B_RC;
    static_assert(!TN || BM == BN, "the TN stager shares one patch shape for both operands");
    using SAK = Stage16KC<BM, BK>;
    using SBK = Stage16KC<BN, BK>;
    using SBR = Stage16RC<BN, BK>;
    constexpr int ROWB = SAK::ROWB, ROWK = SBR::ROWK;
    constexpr int LDS_A = A_RC ? Stage16RC<BM, BK>::LDS_BYTES : SAK::LDS_BYTES;
    constexpr int LDS_B = B_RC ? SBR::LDS_BYTES : SBK::LDS_BYTES;
    constexpr int MI = BM / 64, NI = BN / 64;
    constexpr int U = (D % 2 == 0) ? D : 2 * D;                 // unroll so that set and LDS-buffer indices are static
    // NT form: the staging loads are issued from inline asm and waited for with hand-counted vmcnt (Stage16KC::wait_loaded).
    // hipcc's own waitcnt insertion answers the ring with vmcnt(0) as soon as the control flow around it is not trivial
    // (e.g. 3 sets with a 6-fold unroll), which drains all sets in flight at every k-tile.
    constexpr bool ASM_LOADS = !A_RC && !B_RC;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const bool producer = threadIdx.x >= 256;                   // wave-uniform
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;      // role-local ids
    char* ldsA = smem;
    char* ldsB = smem + 2 * LDS_A;
    float* red = reinterpret_cast<float*>(smem + 2 * LDS_A + 2 * LDS_B);      // bias-grad partials: own region, so the
    constexpr int KP = BK / 8, RP = BM / 8;                                     // next tile's staging never overwrites them
    // PERSISTENT tile loop: a launch has at most chip-filling size; workgroup b walks tiles b, b + grid, ...  Both
    // roles see the same tile sequence and the same number of barriers per tile.  The producers of tile t+1 start as
    // soon as the last k-tile of t has been multiplied, i.e. they fetch under the consumers' epilogue of tile t.
    const int total_tiles = (int)gridDim.x;
    M2F_TS(0);
  for (int bpos = xcd_remap((int)blockIdx.x, (int)gridDim.x); bpos < total_tiles; bpos += (int)gridDim.x) {
    int pi = 0;
#pragma unroll
    for (int i = 1; i < M2F_GEMM_MAX_PROBLEMS; ++i)
        if (bpos >= gb.tb[i]) pi = i;                            // unused slots hold INT_MAX
    const GemmProblem& P = gb.pr[pi];                            // epilogue terms (consumers, off the critical path)
    const GemmHot Hh = gb.hot[pi];                               // descriptors the first loads depend on: the compact header
    const int M = Hh.M, N = Hh.N;
    const int tl = bpos - Hh.tile_begin;
    const int tiles_m = (M + BM - 1) / BM;
    const int m0 = (tl % tiles_m) * BM, n0 = (tl / tiles_m) * BN;       // M fastest: neighbours share the B panel
    const int nk0 = (Hh.k[0] + BK - 1) / BK, nk = nk0 + (Hh.k[1] + BK - 1) / BK;
    const bool has_bg = TN && Hh.has_bias_grad && n0 == 0;              // block-uniform

    if (producer) {
        // ================================ PRODUCER: global -> registers -> LDS ================================
        const uint32_t flags = Hh.flags;
        const bool reluA = flags & GF_RELU_A, reluB = flags & GF_RELU_B;
        struct Set {                   // one register set = this thread's share of one k-tile of both operands
            SAK ak;                    // NT, NN: A
            SBK bk;                    // NT: B
            SBR br;                    // NN: B (threads 0..127) | TN: A (threads 0..127) or B (threads 128..255)
        };
        Set sets[D];
        int cur_seg = -1;
        const bool second_half = tid >= 128;
        float colsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool want_bg = has_bg && !second_half;
        // operand descriptors in SGPRs for the whole k-loop: indexing P.a.q[seg] with a run-time seg makes the compiler
        // re-read the kernarg segment (s_load + lgkmcnt(0)) several times per k-tile, serialised in front of the loads
        const uint16_t* const aq0 = Hh.aq[0]; const uint16_t* const aq1 = Hh.aq[1];
        const uint16_t* const bq0 = Hh.bq[0]; const uint16_t* const bq1 = Hh.bq[1];
        const int ak0 = Hh.k[0], ak1 = Hh.k[1];
        const int ald0 = Hh.ldaq[0], ald1 = Hh.ldaq[1], bld0 = Hh.ldbq[0], bld1 = Hh.ldbq[1];
        auto setup_all = [&](int seg) {
            const int lda = seg ? ald1 : ald0, ldb = seg ? bld1 : bld0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                if constexpr (!A_RC) sets[i].ak.setup(lda, M, m0, tid);
                if constexpr (!B_RC) sets[i].bk.setup(ldb, N, n0, tid);
                if constexpr (!A_RC && B_RC) sets[i].br.setup(ldb, N, n0, tid);
                if constexpr (TN) {
                    if (second_half) sets[i].br.setup(ldb, N, n0, tid - 128);
                    else sets[i].br.setup(lda, M, m0, tid);
                }
            }
        };
        auto issue = [&](Set& st, int kt_raw) {                 // unconditional: past-the-end tiles are fully masked
            const bool tv = kt_raw < nk;
            const int kt = tv ? kt_raw : 0;
            const int seg = kt >= nk0 ? 1 : 0;
            const int kbase = (seg ? kt - nk0 : kt) * BK;
            if (seg != cur_seg) { setup_all(seg); cur_seg = seg; }   // wave-uniform, at most twice
            const int ks = tv ? (seg ? ak1 : ak0) : 0;
            const uint16_t* const qa = seg ? aq1 : aq0;
            const uint16_t* const qb = seg ? bq1 : bq0;
            if constexpr (ASM_LOADS) {
                st.ak.template issue<true>(qa, ks, kbase);
                st.bk.template issue<true>(qb, ks, kbase);
                return;
            }
            if constexpr (!A_RC) st.ak.issue(qa, ks, kbase);
            if constexpr (!B_RC) st.bk.issue(qb, ks, kbase);
            if constexpr (!A_RC && B_RC) st.br.issue(qb, ks, kbase);
            if constexpr (TN) st.br.issue(second_half ? qb : qa, ks, kbase);
        };
        auto store = [&](Set& st, int buf) {
            if constexpr (ASM_LOADS) {
                // every round issues one set and stores one: D - 1 whole sets are younger than the one stored now
                constexpr int PER_SET = SAK::NT + SBK::NT;
                st.ak.template wait_loaded<(D - 1) * PER_SET + SBK::NT>();
                st.bk.template wait_loaded<(D - 1) * PER_SET>();
            }
            if constexpr (!A_RC) st.ak.store(ldsA + buf * LDS_A, reluA);
            if constexpr (!B_RC) st.bk.store(ldsB + buf * LDS_B, reluB);
            if constexpr (!A_RC && B_RC) { float dummy[8]; st.br.store(ldsB + buf * LDS_B, reluB, false, dummy); }
            if constexpr (TN) {
                if (second_half) { float dummy[8]; st.br.store(ldsB + buf * LDS_B, reluB, false, dummy); }
                else st.br.store(ldsA + buf * LDS_A, reluA, want_bg, colsum);
            }
        };

        M2F_TS(1);
#pragma unroll
        for (int i = 0; i < D; ++i) issue(sets[i], i);
        M2F_TS(2);
        store(sets[0], 0);
        M2F_TS(3);
        lds_barrier();                                          // (B0) tile 0 visible
        issue(sets[0], D);
        M2F_TS(4);
        // The loop is LEFT (not skipped through) when the k-tiles run out: a path that skips the rest of an unrolled round
        // and still reaches the loop header carries a different number of outstanding loads, and the waitcnt pass then
        // answers every wait at the header with vmcnt(0) - draining the ring once per round.
        for (int kt0 = 0;; kt0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kt = kt0 + u;
                if (kt >= nk) goto k_tiles_done;                 // block-uniform
                store(sets[(u + 1) % D], (u + 1) & 1);           // tile kt+1 (all-zero past the end) while tile kt is multiplied
                lds_barrier();                                   // (B1 per tile)
                issue(sets[(u + 1) % D], kt + 1 + D);
            }
        }
k_tiles_done:
        if constexpr (TN) {
            if (has_bg) {
                // threads 0..127 hold column sums of their 8 rows over their k-group: red[kp][row], then fixed-order sum
                if (!second_half) {
                    const int kp = tid / RP, rp = tid % RP;
#pragma unroll
                    for (int e = 0; e < 8; ++e) red[kp * BM + 8 * rp + e] = colsum[e];
                }
                lds_barrier();                                   // (B2)
            }
        }
        M2F_TS(5);
        continue;                                               // next tile (every issued load was consumed or is dead)
    }

    // ==================================== CONSUMER: LDS -> MFMA -> epilogue ====================================
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf) {
        const char* aimg = ldsA + buf * LDS_A;
        const char* bimg = ldsB + buf * LDS_B;
        const char* ab = aimg + (wm * (BM / 2) + (lane & 31)) * ROWB + (lane >> 5) * 16;      // row-major images
        const char* bb = bimg + (wn * (BN / 2) + (lane & 31)) * ROWB + (lane >> 5) * 16;
        if constexpr (FP8) {
            // row = 2*BK e4m3 values; slice ks covers 16 of them: lane (row, half) holds bytes [16*ks + 8*half, +8)
            constexpr int KS8 = BK / 8;
            const char* a8 = aimg + (wm * (BM / 2) + (lane & 31)) * ROWB + (lane >> 5) * 8;
            const char* b8 = bimg + (wn * (BN / 2) + (lane & 31)) * ROWB + (lane >> 5) * 8;
#pragma unroll
            for (int g0 = 0; g0 < KS8; g0 += 4) {
                long fa[4][MI], fb[4][NI];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                    for (int i = 0; i < MI; ++i) fa[kk][i] = *reinterpret_cast<const long*>(a8 + i * 32 * ROWB + (g0 + kk) * 16);
#pragma unroll
                    for (int j = 0; j < NI; ++j) fb[kk][j] = *reinterpret_cast<const long*>(b8 + j * 32 * ROWB + (g0 + kk) * 16);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NI; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
        // all fragments of the k-tile first (one exposed LDS latency per tile instead of one per 16-wide k-slice), then
        // the MFMA run back to back
        constexpr int KS = BK / 16;
        bf16x8 a[KS][MI], b[KS][NI];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                if constexpr (A_RC) a[ks][i] = frag_from_kmajor(aimg, ROWK, wm * (BM / 2) + i * 32, 16 * ks, lane);
                else a[ks][i] = *reinterpret_cast<const bf16x8*>(ab + i * 32 * ROWB + ks * 32);
            }
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                if constexpr (B_RC) b[ks][j] = frag_from_kmajor(bimg, ROWK, wn * (BN / 2) + j * 32, 16 * ks, lane);
                else b[ks][j] = *reinterpret_cast<const bf16x8*>(bb + j * 32 * ROWB + ks * 32);
            }
        }
        __builtin_amdgcn_sched_barrier(0);          // keep the reads ahead of the MFMA run (the scheduler sinks them otherwise)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ks][i], b[ks][j], acc[i][j], 0, 0, 0);
    };

    M2F_TS(1);
    lds_barrier();                                              // (B0)
    M2F_TS(2);
    for (int kt0 = 0; kt0 < nk; kt0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kt0 + u < nk) {                                  // block-uniform
                compute(u & 1);
                lds_barrier();                                   // (B1 per tile)
            }
        }
    }
    if constexpr (TN) {
        if (has_bg) {
            lds_barrier();                                       // (B2) producers' partial sums are in LDS
            if (tid < BM) {
                float sum = 0.f;
                for (int q = 0; q < KP; ++q) sum += red[q * BM + tid];
                // (GF_ACCUM, the accumulate form of a weight gradient: the bias gradient accumulates with C - old + new, as C does)
                if (m0 + tid < M) P.bias_grad[m0 + tid] = (P.flags & GF_ACCUM) ? P.bias_grad[m0 + tid] + sum : sum;
            }
        }
    }
    M2F_TS(3);
    gemm_epilogue<MI, NI, BM, BN, GELU, FP8, true>(gb, P, acc, m0, n0, lane, wm, wn);
    M2F_TS(4);
  }
}

// Two register budgets of the same body.  "wide": up to 256 VGPRs, one workgroup (8 waves) per CU - the launches with
// at most one tile per CU, where a deep load ring is what matters.  "dense": at most 128 VGPRs (4 waves per SIMD), two
// workgroups per CU with a shallower ring each - the launches with more tiles than CUs.
template <bool A_RC, bool B_RC, int BM, int BN, int BK, int D, bool GELU = false, bool FP8 = false>
__global__ __launch_bounds__(512) void m2f_gemm16_kernel(const GemmBatch gb) {
    gemm16_body<A_RC, B_RC, BM, BN, BK, D, GELU, FP8>(gb);
}
template <bool A_RC, bool B_RC, int BM, int BN, int BK, int D>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void m2f_gemm16_dense_kernel(const GemmBatch gb) {
    gemm16_body<A_RC, B_RC, BM, BN, BK, D>(gb);
}

template <bool A_RC, bool B_RC, int BM, int BN, int BK, int D, bool DENSE = false, bool GELU = false, bool FP8 = false>
hipError_t launch_cfg16(const GemmBatch& gb, int total_tiles, hipStream_t stream) {
    constexpr int lds = 2 * (A_RC ? Stage16RC<BM, BK>::LDS_BYTES : Stage16KC<BM, BK>::LDS_BYTES) +
                        2 * (B_RC ? Stage16RC<BN, BK>::LDS_BYTES : Stage16KC<BN, BK>::LDS_BYTES) + (BK / 8) * BM * 4;
    static_assert(lds <= 160 * 1024, "LDS budget");
    static_assert(!DENSE || 2 * lds <= 160 * 1024, "two workgroups per CU");
    GemmBatch hb = gb;                                          // compact header for the kernel's critical path
    m2f_gemm_fill_hot(hb, true);
    void (*kern)(const GemmBatch);
    static_assert(!(DENSE && GELU), "the GELU epilogue exists for the wide forward-form kernels only");
    if constexpr (DENSE) kern = m2f_gemm16_dense_kernel<A_RC, B_RC, BM, BN, BK, D>;
    else kern = m2f_gemm16_kernel<A_RC, B_RC, BM, BN, BK, D, GELU, FP8>;
    if (lds > 64 * 1024) {
        static bool attr_set = false;
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(total_tiles), dim3(512), lds, stream, hb);
    return hipGetLastError();
}

template <int PREC, bool A_RC, bool B_RC, int BM, int BN, int BK, bool VEC, bool GELU = false>
hipError_t launch_cfg(const GemmBatch& gb, int total_tiles, hipStream_t stream) {
    using SA = Stage<PREC, A_RC, BM, BK, VEC>;
    using SB = Stage<PREC, B_RC, BN, BK, VEC>;
    constexpr int lds = 2 * SA::LDS_BYTES + 2 * SB::LDS_BYTES;
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = m2f_gemm_kernel<PREC, A_RC, B_RC, BM, BN, BK, VEC, GELU>;
    if (lds > 64 * 1024) {
        static bool attr_set = false;
        if (!attr_set) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) return e;
            attr_set = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3(total_tiles), dim3(256), lds, stream, gb);
    return hipGetLastError();
}

// The instantiations.  The kernel set is closed: a flag that has no kernel of its own (GELU outside the forward form) folds onto the
// kernel without it, as the launches always did.
constexpr int bk_f32src(int prec, int tile) { return prec == M2F_PREC_F32 ? (tile == 128 ? 32 : 64) : (tile == 128 ? 64 : 128); }

template <int PREC, bool A_RC, bool B_RC>
hipError_t launch_tile(const GemmBatch& gb, bool tile128, bool vec, bool gelu, int t, hipStream_t stream) {
    return m2f_pick_bools([&](auto T128, auto VEC, auto GELU) {
        constexpr int T = T128.value ? 128 : 64;
        constexpr bool G = GELU.value && !A_RC && !B_RC;        // GELU epilogue: forward form only (text encoder)
        return launch_cfg<PREC, A_RC, B_RC, T, T, bk_f32src(PREC, T), VEC.value, G>(gb, t, stream);
    }, tile128, vec, gelu);
}

template <bool A_RC, bool B_RC>
hipError_t launch_tile16(const GemmBatch& gb, int tile, bool gelu, bool fp8, int t, hipStream_t stream) {
    if constexpr (!A_RC && !B_RC) {     // forward form only: 256x128 tiles, the GELU epilogue (text encoder), e4m3 operands - own instantiations
        if (tile == 256 || tile == 128)
            return m2f_pick_bools([&](auto BIG, auto GELU, auto FP8) {
                return launch_cfg16<false, false, BIG.value ? 256 : 128, 128, 64, BIG.value ? 2 : 3, false, GELU.value, FP8.value>(gb, t, stream);
            }, tile == 256, gelu, fp8);
        if (gelu) return launch_cfg16<false, false, 64, 64, 128, 2, false, true>(gb, t, stream);
    }
    if (tile == 128) return launch_cfg16<A_RC, B_RC, 128, 128, 64, 3>(gb, t, stream);
    // ONE 64x64 build for every launch size: ring depth 2 within 128 VGPRs (two workgroups per CU when the launch has more
    // tiles than CUs).  Deeper rings gain nothing for these launches (start-up and dispatch bound, not ring bound) and cost
    // code size: same-box A/B of the whole step 2.130 (depth 4 + separate 256-VGPR build) -> 2.107 ms, and again after the
    // ring kept its loads in flight: 2.34 / 2.38 (depth 3 / 4, 256-VGPR build for launches of
    // at most 256 tiles) vs 2.32 ms; the step alternates between ~8 kernels, so every kilobyte of code is instruction-cache
    // traffic at each launch.
    return launch_cfg16<A_RC, B_RC, 64, 64, 128, M2F_CHAIN_D, true>(gb, t, stream);
}

// NT, NN or TN as compile-time flags (A_RC without B_RC does not exist)
template <typename F>
hipError_t pick_layout(bool a_rc, bool b_rc, F&& f) {
    if (!b_rc) return f(std::false_type{}, std::false_type{});
    if (!a_rc) return f(std::false_type{}, std::true_type{});
    return f(std::true_type{}, std::true_type{});
}

// fp32-source launches: tiles numbered with the split-K bookkeeping - `splitk` consecutive workgroups share one output tile, each
// problem takes at most the wanted factor and at least two k-tiles per slice; slab_begin in slices (one [BM x BN] partial each),
// cnt_begin in tiles (one ticket each).  (A scratch too small for the wish arrives here as ch.splitk = 1: the chooser's fallback.)
int number_tiles_splitk(GemmBatch& gb, int tile, int bk, int want_s) {
    int t = 0, tiles_total = 0;
    for (int i = 0; i < gb.count; ++i) {
        GemmProblem& p = gb.pr[i];
        p.splitk = m2f_gemm_splitk_of(p, want_s, bk);
        p.tile_begin = t;
        p.slab_begin = t;
        p.cnt_begin = tiles_total;
        p.tiles_n = m2f_cdiv(p.N, tile);
        const int tiles = m2f_cdiv(p.M, tile) * p.tiles_n;
        t += tiles * p.splitk;
        tiles_total += tiles;
    }
    return t;
}

}  // namespace

#ifdef M2F_EXP_TIMING
extern "C" int m2f_dbg_read(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(m2f_dbg), sizeof(unsigned long long) * 64);
}
#endif

// Executes a choice of one of the register-staged forms (gemm_dispatch.hip: m2f_gemm_choose / m2f_gemm_choose_fp8): numbers the tiles
// and switches to the instantiation.
hipError_t m2f_launch_gemm_staged(GemmBatch& gb, const GemmChoice& ch, int prec, int layout, hipStream_t stream) {
    const int form = ch.form & 0xFF;
    const bool a_rc = !ch.b_t && layout == M2F_LAYOUT_TN, b_rc = !ch.b_t && layout != M2F_LAYOUT_NT;
    bool gelu = false;
    for (int i = 0; i < gb.count; ++i) gelu = gelu || (gb.pr[i].flags & GF_GELU_OUT);
    if (form > M2F_FORM_F32SRC_SPLITK) {                        // bf16-source (or e4m3) kernels
        const int t = m2f_gemm_number_tiles(gb, ch.tile_m, ch.tile_n);
        if (t == 0) return hipSuccess;
        const bool fp8 = form == M2F_FORM_FP8_128x128 || form == M2F_FORM_FP8_256x128;
        return pick_layout(a_rc, b_rc, [&](auto A, auto B) { return launch_tile16<A.value, B.value>(gb, ch.tile_m, gelu, fp8, t, stream); });
    }
    const int t = number_tiles_splitk(gb, ch.tile_m, bk_f32src(prec, ch.tile_m), ch.splitk);
    if (t == 0) return hipSuccess;
    const bool vec = ch.form & M2F_FORM_VEC;                    // 16-byte loads: every operand of every problem allows them
    return pick_layout(a_rc, b_rc, [&](auto A, auto B) {
        if (prec == M2F_PREC_F32) return launch_tile<M2F_PREC_F32, A.value, B.value>(gb, ch.tile_m == 128, vec, gelu, t, stream);
        return launch_tile<M2F_PREC_BF16, A.value, B.value>(gb, ch.tile_m == 128, vec, gelu, t, stream);
    });
}
