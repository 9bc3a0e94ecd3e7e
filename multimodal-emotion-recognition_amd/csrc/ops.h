// Internal launch interfaces of the gfx950 kernels (host side). The public C ABI is include/m2fnet_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/m2fnet_hip.h"

// ------------------------------------------------------------------------------------------------
// Grouped GEMM:  C[M,N] = epilogue( sum_k A(m,k) * B(n,k) )
//   operand layouts   KC: element (row, k) at p[row*ld + k]   (k contiguous)
//                     RC: element (row, k) at p[k*ld + row]   (row contiguous)
//   forward  Y  = X W^T        A = X  KC, B = W  KC
//   dgrad    dX = dY W         A = dY KC, B = W  RC   (reduction over W's row index)
//   wgrad    dW = dY^T X       A = dY RC, B = X  RC   (reduction over tokens)
//   Each operand may be the concatenation of two segments along k (cat(x, text) of the FAM layer,
//   src/model.py:16, is never materialised).
//   epilogue order: +bias[n] -> relu -> dropout(site) -> +res[m,n] -> *(gate[m,n] > 0 ? gate_scale : 0)
//                   -> (C += | C =)
// ------------------------------------------------------------------------------------------------
enum { M2F_PREC_F32 = 0, M2F_PREC_BF16 = 1 };
enum { M2F_LAYOUT_NT = 0, M2F_LAYOUT_NN = 1, M2F_LAYOUT_TN = 2 };   // fwd / dgrad / wgrad
enum {
    GF_RELU_A = 1, GF_RELU_B = 2, GF_RELU_OUT = 4, GF_ACCUM = 8,
    GF_VEC_A = 16, GF_VEC_B = 32,    // set by the launcher when 16-byte loads are legal
    GF_GELU_OUT = 64,                // exact (erf) GELU instead of ReLU in the epilogue (RoBERTa's intermediate.dense)
    GF_NO_BF16 = 256,                // bf16 mode: nobody stages C from its bf16 shadow (a residual term, a LayerNorm input): the ring epilogue skips it
    GF_NO_F32 = 128                  // bf16 mode: nobody reads C as fp32 (plan_build.hip::mark_unread_fp32) - a kernel that writes C's bf16 shadow
                                     // may leave the fp32 copy unwritten (the ring epilogue does; the other kernels ignore the flag)
    // (fp8 launches, m2f_launch_gemm_fp8: a.q / b.q point at e4m3 bytes, k / ldq count BYTE PAIRS, the accumulator is
    //  multiplied by acc_scale = 1 / (scale_a * scale_b) before the epilogue terms)
};

struct GemmOperand {
    const float* p[2];
    int ld[2];
    int k[2];          // reduction length of each segment (k[1] == 0: single segment)
    // bf16 shadow of the same data (bf16 mode): same logical element (row, k), own leading dimension; the columns
    // between the logical width and ldq are zero.  null = no shadow (the launch then stages from fp32).
    const uint16_t* q[2];
    int ldq[2];
    // B operand of the dgrad form only: bf16 shadow of the TRANSPOSED matrix (element (row, k) at qt[row*ldqt + k]),
    // which lets the launch run as the k-contiguous (forward) form.  null = not available.
    const uint16_t* qt[2];
    int ldqt[2];
};

// bf16 shadows of workspace activations: element i of the fp32 workspace has its shadow at shadow[i] (activation
// buffers use leading dimensions that are multiples of 8, so shadows keep 16-byte row alignment).  Producer kernels
// write both copies; ws_base == null disables shadow writes.
struct ShadowMap {
    const float* ws_base;
    uint16_t* shadow;
    size_t ws_floats;
};

struct GemmProblem {
    GemmOperand a, b;
    float* c;
    const float* bias;        // [N] or null
    const float* res;         // [M, N] (ldres) or null
    const float* gate;        // [M, N] (ldgate) or null
    float* bias_grad;         // wgrad only: [M] column sums of A over the reduction dim, or null
    int M, N, ldc, ldres, ldgate;
    float gate_scale;
    float acc_scale;          // fp8 launches only: de-quantisation factor applied to the accumulator
    uint8_t* c8;              // fp8 launches only (nullable): the result goes out as e4m3(v * c8_scale) at c8[m*ldc + n]
    float c8_scale;           //   INSTEAD of fp32 C (an activation whose only reader is the next fp8 GEMM)
    uint32_t drop_site;       // 0 = no dropout in the epilogue
    uint32_t flags;
    int tile_begin, tiles_n;  // filled by the launcher
    int splitk, slab_begin, cnt_begin;   // filled by the launcher (k-slices per tile, first partial slab, first ticket)
};

#define M2F_GEMM_MAX_PROBLEMS 8
// What a workgroup of the bf16-source kernel needs before it can issue its first load, packed at the FRONT of the kernarg
// block (filled by the launcher from pr[]): the tile -> problem search reads one 32-byte array instead of eight fields in
// eight different 256-byte structs, the producer's descriptors sit in 96 contiguous bytes instead of five cache lines of a
// cold kernarg segment.
struct GemmHot {
    const uint16_t* aq[2]; const uint16_t* bq[2];
    int M, N, k[2], ldaq[2], ldbq[2];
    uint32_t flags; int tile_begin; int has_bias_grad; int pad_[3];
};
struct GemmBatch {
    int tb[M2F_GEMM_MAX_PROBLEMS];           // tile_begin of problem i (INT_MAX for unused slots)
    GemmHot hot[M2F_GEMM_MAX_PROBLEMS];
    GemmProblem pr[M2F_GEMM_MAX_PROBLEMS];
    int count;
    const uint32_t* rng;      // dropout RNG state (device), may be null when no problem has drop_site
    uint32_t drop_thresh;     // p * 2^32
    float drop_scale;         // 1 / (1 - p)
    // split-K scratch (optional; null = never split): partial-tile slabs [splitk_max_tiles * 4][64*64] floats and one
    // zero-initialised ticket per tile (the last arriver re-arms it)
    float* splitk_ws;
    unsigned* splitk_cnt;
    int splitk_max_tiles;
    ShadowMap sh;             // C (when it lies in the workspace) is also written as bf16
    // TABLE form (m2f_launch_gemm_table): the problems live in device memory, table[i]; pr[] / count are unused in this form.
    // Every workgroup walks its OWN tile list, tile_rec[wg_begin[b] .. wg_begin[b + 1]) for workgroup b of a grid of wg_count;
    // a record = problem | m-tile << 16 | n-tile << 24 (m2f_gemm_table_walk)
    const GemmProblem* table;
    int total_tiles;
    bool table_p8;            // 256 x 256 tiles on the eight-phase schedule (gemm_p8.h); false: 256 x 128 ring tiles (gemm_ring.h)
    const uint32_t* tile_rec;
    const int* wg_begin;
    int wg_count;
    // eight-phase form (gemm_p8.h): start skew - estimated cycles per k-tile (0 = off; bit 30: also workgroups without slack) and the
    // longest tile list of any workgroup of the launch
    int p8_skew, p8_max_tiles;
    // eight-phase table form with the optimizer in its epilogue (EPI 3, round 4): the tile that holds a weight gradient in registers
    // applies torch.optim.Adam's update to its parameter elements - dW never reaches memory.  Device pointer (scalar loads), null = off.
    // Per problem: res = (float*) bf16 shadow W of the problem's first element, gate = (float*) shadow W^T of it, ldres / ldgate their leading
    // dimensions (pad8(cols), pad8(rows of the whole tensor)).
    const struct M2FAdamFuse* adam;
};
struct M2FAdamFuse {
    float* p; const float* g_base; float* m; float* v;      // flat parameter / gradient / moment buffers, same indexing; the problems' c points into g_base
    const float* hyper;                                     // device: lr / bc1, beta1, beta2, eps, weight_decay, 1 / sqrt(bc2) (m2f_launch_adam_hyper)
    const float* gs_ptr;                                    // nullable device scalar: gradients are divided by it (global valid-utterance denominator)
};
#define M2F_SPLITK_MAX_TILES 512

// ---- GEMM dispatch (gemm_dispatch.hip): which kernel form a launch takes ------------------------------------------------------
// The knobs of that policy, read from the environment once, at first use (defaults and their measured reasons: m2f_gemm_knobs)
struct GemmKnobs {
    int ring, ring_min, ring64_min, ring32_min, ring256_min, ring256_2r;      // M2F_RING, _RING_MIN, _RING64_MIN, _RING32_MIN, _RING256_MIN, _RING256_2R
    int p8, p8_min, ring_fp8, skinny;                                         // M2F_P8, M2F_P8_MIN, M2F_RING_FP8, M2F_SKINNY
};
const GemmKnobs& m2f_gemm_knobs();
// What the chooser decides for one launch; the launchers only execute it.
struct GemmChoice {
    int form;              // the complete M2F_FORM_* value, M2F_FORM_VEC / _SRC16 / _NN_T included (M2F_FORM_NONE: nothing to launch)
    int tile_m, tile_n;
    bool src16;            // every operand is staged from its bf16 shadow (no kernel of the launch reads the fp32 originals)
    bool b_t;              // NN launch run as the k-contiguous form: B is taken through its transposed shadow (qt / ldqt)
    int splitk;            // wanted split-K factor (1: none); a problem takes min(splitk, k-tiles / 2)
};
// Pure: no HIP call, nothing written, no global read but the knobs.  m2f_gemm_choose expects a validated batch (m2f_launch_gemm);
// the fp8 chooser sees k / ldq in BYTES, as m2f_gemm_fp8 passes them (before the launcher halves them into byte pairs).
GemmChoice m2f_gemm_choose(const GemmBatch& gb, int prec, int layout, int tile);
GemmChoice m2f_gemm_choose_fp8(const GemmBatch& gb);
extern int m2f_g_last_form;        // host-side record of the kernel form the last GEMM launch took (M2F_FORM_*); dispatched launches: set in gemm_execute
extern long long m2f_g_ring_launches;         // host-side count of ring-form and eight-phase launches
bool m2f_gemm_stages_bf16(const GemmBatch& gb, int layout);      // host: does the bf16-mode launch read bf16 shadows only?  (the chooser's answer)
// eligibility (b_t: B's shadow is the transposed one): the ring forms, the 256x128 ring form (bias / ReLU / GELU / residual epilogues
// only), the eight-phase 256x256 form (that epilogue set, single segment, k % 64 == 0)
bool m2f_gemm_ring_ok(const GemmBatch& gb, bool b_t = false);
bool m2f_gemm_ring256_ok(const GemmBatch& gb, bool b_t = false);
bool m2f_gemm_p8_ok(const GemmBatch& gb, bool b_t = false);
// the launchers a choice is executed by
hipError_t m2f_launch_gemm_skinny(const GemmBatch& gb, const GemmChoice& ch, int prec, hipStream_t stream);      // skinny.hip
hipError_t m2f_launch_gemm_staged(GemmBatch& gb, const GemmChoice& ch, int prec, int layout, hipStream_t stream);      // gemm.hip: register-staged kernels
hipError_t m2f_launch_gemm_ring(GemmBatch& gb, int bm, int bn, hipStream_t stream);      // gemm_ring_<bm>x<bn>.hip
hipError_t m2f_ring_launch_256x128_fp8(GemmBatch& gb, hipStream_t stream);                 // gemm_ring_256x128_fp8.hip
hipError_t m2f_ring_launch_table_rc_256x128(const GemmBatch& gb, hipStream_t stream);      // the table form, 256 x 128 tiles (gemm_ring_table.hip)
hipError_t m2f_ring_launch_table_rc_256x128_acc(const GemmBatch& gb, hipStream_t stream);  // ... its accumulate form, old + new (gemm_ring_table_acc.hip)
hipError_t m2f_p8_launch_kc(GemmBatch& gb, hipStream_t stream);                            // gemm_p8.hip
hipError_t m2f_p8_launch_kc_fp8(GemmBatch& gb, hipStream_t stream);
hipError_t m2f_p8_launch_table_rc(const GemmBatch& gb, hipStream_t stream);
hipError_t m2f_p8_launch_table_rc_adam(const GemmBatch& gb, hipStream_t stream);     // Adam in the epilogue (gb.adam)
// ... with parameter groups (EPI 6): as above, and every problem carries the hyper-table row of its tensor's group in `c8` (a const float*;
// fp8 launches alone use that field otherwise) - gb.adam->hyper is not read; the update multiplies the parameter by the row's `decay` first
hipError_t m2f_p8_launch_table_rc_adam_grouped(const GemmBatch& gb, hipStream_t stream);
hipError_t m2f_p8_launch_table_rc_acc(const GemmBatch& gb, hipStream_t stream);      // accumulate form: dW, bias gradients = old + new

// Numbers the tiles of a grouped launch of bm x bn tiles without split-K (tile_begin, tiles_n of every problem) -> tiles of the launch
static inline int m2f_gemm_number_tiles(GemmBatch& gb, int bm, int bn) {
    int t = 0;
    for (int i = 0; i < gb.count; ++i) {
        GemmProblem& p = gb.pr[i];
        p.splitk = 1; p.slab_begin = 0; p.cnt_begin = 0;
        p.tile_begin = t;
        p.tiles_n = (p.N + bn - 1) / bn;
        t += ((p.M + bm - 1) / bm) * p.tiles_n;
    }
    return t;
}
// split-K factor a problem takes under the launch's wish `want`: at least two k-tiles (of bk) per slice
static inline int m2f_gemm_splitk_of(const GemmProblem& p, int want, int bk) {
    const int nk = (p.a.k[0] + bk - 1) / bk + (p.a.k[1] + bk - 1) / bk;
    const int sp = want < nk / 2 ? want : nk / 2;
    return sp < 1 ? 1 : sp;
}
// Fills the compact header of the launcher's own copy of a numbered batch (tb[], hot[]) from its pr[]; has_bias_grad: the kernel
// can emit one (the ring forms cannot and pass false)
static inline void m2f_gemm_fill_hot(GemmBatch& hb, bool has_bias_grad) {
    for (int i = 0; i < M2F_GEMM_MAX_PROBLEMS; ++i) {
        hb.tb[i] = i < hb.count ? hb.pr[i].tile_begin : 0x7fffffff;
        GemmHot& h = hb.hot[i];
        memset(&h, 0, sizeof(h));
        if (i >= hb.count) continue;
        const GemmProblem& p = hb.pr[i];
        h.aq[0] = p.a.q[0]; h.aq[1] = p.a.q[1]; h.bq[0] = p.b.q[0]; h.bq[1] = p.b.q[1];
        h.M = p.M; h.N = p.N; h.k[0] = p.a.k[0]; h.k[1] = p.a.k[1];
        h.ldaq[0] = p.a.ldq[0]; h.ldaq[1] = p.a.ldq[1]; h.ldbq[0] = p.b.ldq[0]; h.ldbq[1] = p.b.ldq[1];
        h.flags = p.flags; h.tile_begin = p.tile_begin; h.has_bias_grad = has_bias_grad && p.bias_grad != nullptr;
    }
}
// host: the bf16 shadow of C when it lies in the shadowed workspace, else null (the skinny kernels take it as an argument)
static inline uint16_t* m2f_gemm_c_shadow(const GemmBatch& gb, const float* c) {
    const ptrdiff_t i = gb.sh.shadow && c >= gb.sh.ws_base ? c - gb.sh.ws_base : -1;
    return (i >= 0 && (size_t)i < gb.sh.ws_floats) ? gb.sh.shadow + i : nullptr;
}

// Launches one grouped GEMM. Returns hipSuccess or the launch error. `tile` = 0 (auto), 64 or 128.
hipError_t m2f_launch_gemm(GemmBatch& gb, int prec, int layout, int tile, hipStream_t stream);
// TABLE form, bf16 mode: the weight-gradient launch dW = dY^T X on the row-major bf16 shadows gb.table[i].{a,b}.q (reduction
// over their rows), optional ReLU on either operand and the bias gradient (column sums of A); plain stores of C.
hipError_t m2f_launch_gemm_table(const GemmBatch& gb, hipStream_t stream);
// the same launch in its accumulate form (m2f_plan_accumulate_grads): every dW element and bias gradient = old + new, one rounded fp32 add
hipError_t m2f_launch_gemm_table_acc(const GemmBatch& gb, hipStream_t stream);
// fp8 (OCP e4m3) operands, forward form only, single problem: C = act(acc_scale * A8 B8^T + bias) + res.  K % 16 == 0,
// lda / ldb % 16 == 0, 16-byte aligned operands.  (SURVEY 8-f4 / BASELINE C5: the text encoder's GEMMs.)
hipError_t m2f_launch_gemm_fp8(GemmBatch& gb, hipStream_t stream);
#ifdef __cplusplus
#include <vector>
bool m2f_gemm_p8_table_ok(const std::vector<GemmProblem>& prs);      // table form of gemm_p8.h: no ReLU on A, single segment
// Per-workgroup tile lists of the ring table forms (tile_m x tile_n tiles: 128x128, 256x128, 256x256) for a grid of n_wg workgroups (workgroup b runs on XCD
// b % 8 under round-robin placement - speed only).  walk = 0: problem by problem, m fastest inside a problem (every round spreads 256
// consecutive tiles - usually of ONE problem - over all eight XCDs, so each L2 pulls its own copy of that problem's
// operands); walk = 1: the tile list is cut into eight contiguous ranges of whole 8 x 4 super-tiles, one per XCD, so a
// problem's operand panels are fetched by one L2 (two at a range boundary) and the 32 tiles an XCD multiplies at a time
// share 8 row panels and 4 column panels.  Returns the number of records (= total tiles), -1 if a problem has more than
// 255 tiles along a dimension.
int m2f_gemm_table_walk(const std::vector<GemmProblem>& prs, int walk, int n_wg, int tile_m, int tile_n, std::vector<uint32_t>& tile_rec, std::vector<int>& wg_begin,
                        const std::vector<int>* only = nullptr);
#endif

// ------------------------------------------------------------------------------------------------
// Attention (one wavefront per (dialogue, head); Q/K/V tiles staged in LDS, fp32 MFMA 16x16x4,
// wavefront-shuffle softmax).  Rows of q/k/v/out are token-major: token t = b*L + i.
// ------------------------------------------------------------------------------------------------
struct AttnProblem {
    const float* q; const float* k; const float* v;   // head h occupies columns [h*hd, (h+1)*hd)
    int ldq, ldk, ldv;
    float* out; int ldo;                               // [T, H*hd]
    float* probs;                                      // [B*H, Lp, Lp] saved P^T (pre-dropout), Lp = 16*ceil(L/16)
    // backward only
    const float* dout; int lddo;
    float* dq; float* dk; float* dv; int lddq, lddk, lddv;
    int H, hd;
    uint32_t drop_site;
    int block_begin;                                   // filled by the launcher
    uint32_t no_f32;                                   // bf16 mode: out (fwd) / dq, dk, dv (bwd) have no fp32 reader - only their bf16 shadows are written
};
#define M2F_ATTN_MAX_PROBLEMS 4
struct AttnBatch {
    int bb[M2F_ATTN_MAX_PROBLEMS];      // block_begin of problem i (INT_MAX for unused slots): one line for the block -> problem search
    AttnProblem pr[M2F_ATTN_MAX_PROBLEMS];
    int count;
    int B, L;
    int band_past;             // context band (below), past side - here and after T: the two fill alignment holes, the struct keeps its size
    const uint8_t* key_pad;    // [B, L], 1 = padded key
    const int* cu;             // PACKED layout (nullable): dialogue b owns token rows cu[b] .. cu[b+1]-1 (at most L of them); key_pad unused
    int T;                     // PACKED layout: token rows of the buffers; rows cu[B] .. T-1 belong to no dialogue and are written as zeros
    // Context band, uniform per launch, stored + 1 so that a zeroed batch means "no band": query i (position inside its dialogue) sees
    // key j iff j is a valid key as ever, and (band_past == 0 or j >= i - (band_past - 1)) and (band_future == 0 or
    // j <= i + (band_future - 1)).  A query that sees no key (a pad slot behind a short dialogue) gets P = 0 and a zero output row.
    int band_future;
    const uint32_t* rng;
    uint32_t drop_thresh;
    float drop_scale;
    ShadowMap sh;              // out (fwd) / dq, dk, dv (bwd) also written as bf16
    bool bwd_fast;             // set by the launcher: the backward takes its one-round-trip path (attention.hip, attn_bwd_fast)
    uint16_t bias_gain16;      // distance-decay bias (below): the upper 16 bits of the fp32 gain, 0 = off - in the hole behind bwd_fast, the struct keeps its size
    int bf16_math;             // bf16 mode, bit mask: 1 = the head-dim contractions (Q K^T, dO V^T) round their operands to bf16 and run
                               // on v_mfma_f32_16x16x32_bf16 (fp32 accumulate): 1/8 of the MFMA instructions at 1/2 the cycles each;
                               // 2 / 4 / 8 / 16 / 32 = the Q / K / V / dO / O slab is staged from the operand's bf16 shadow (half the bytes)
    // Speaker heads (below), forward only: one id per token row, in the rows' own order (padded: [B, L] as key_pad; packed: row cu[b] + i),
    // and how many heads of every problem are same-speaker / other-speaker heads.  null / (0, 0) = off.  Appended: every field above
    // keeps its offset, the struct grew from 648 to 664 bytes (attention.hip's kernarg warm-up covers 768).
    const uint8_t* speaker;
    uint8_t spk_same, spk_other;
};
// Speaker heads: the class of head h under (n_same, n_other) - heads 0 .. n_same - 1 see the keys of the query's own speaker only (the
// utterance itself always qualifies), the next n_other heads the keys of every OTHER speaker only, the rest are untouched.  The one
// definition: every kernel that tests a speaker and every host check calls it.
enum { M2F_SPK_NONE = 0, M2F_SPK_SAME = 1, M2F_SPK_OTHER = 2 };
__host__ __device__ inline int m2f_attn_speaker_class(int h, int n_same, int n_other) {
    return h < n_same ? M2F_SPK_SAME : (h < n_same + n_other ? M2F_SPK_OTHER : M2F_SPK_NONE);
}
// host: a launch with speaker heads carries the ids, and its counts fit every problem's heads (the launchers refuse the others)
inline bool m2f_attn_speakers_ok(const AttnBatch& ab) {
    if (!(ab.spk_same | ab.spk_other)) return true;
    if (!ab.speaker) return false;
    for (int i = 0; i < ab.count && i < M2F_ATTN_MAX_PROBLEMS; ++i)
        if ((int)ab.spk_same + (int)ab.spk_other > ab.pr[i].H) return false;
    return true;
}
inline void m2f_attn_set_band(AttnBatch& ab, int past, int future) {      // (past, future): >= 0, or negative = unlimited
    const int cap = 1 << 20;                                               // (far beyond any L: the same band, and i +- it cannot overflow)
    ab.band_past = past < 0 ? 0 : (past < cap ? past : cap) + 1;
    ab.band_future = future < 0 ? 0 : (future < cap ? future : cap) + 1;
}
// Distance-decay bias (ALiBi), uniform per launch: a visible key's score is fma(-slope, float(|i - j|), dot * 1/sqrt(hd)) in fp32, i and
// j the positions the band compares.  slope = gain * base(h, H): with n = 2^floor(log2 H), base = 2^(-8 (h + 1) / n) for h < n and
// 2^(-4 (2 (h - n) + 1) / n) behind (the recipe for head counts that are no power of two).  The gain travels as the upper half of its
// fp32 value (what a bf16 holds), so a zeroed batch means "no bias"; the applied gain is the requested one rounded to bf16.  The one
// definition: every kernel that forms a score (attention.hip, attention_dlong.hip, attention_stream.hip, attention_stream_chunk.hip)
// calls it, and adds the term with an explicit __fmaf_rn.  The backward kernels read the saved probabilities and never see it.
__host__ __device__ inline float m2f_attn_bias_slope(int h, int H, float gain) {
    int n = 1;
    while (2 * n <= H) n *= 2;
    const float e = h < n ? -8.0f * (float)(h + 1) / (float)n : -4.0f * (float)(2 * (h - n) + 1) / (float)n;
    return gain * exp2f(e);
}
inline uint16_t m2f_attn_bias_gain16(float gain) {                         // fp32 -> the stored half, round to nearest even (gain finite, >= 0)
    const uint32_t u = __builtin_bit_cast(uint32_t, gain);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float m2f_attn_bias_gain(uint16_t g16) { return __builtin_bit_cast(float, (uint32_t)g16 << 16); }
// bit jl = the band lets query i see key kb + jl (jl = 0 .. 63); all ones without a band
__host__ __device__ inline unsigned long long m2f_attn_band_bits(const AttnBatch& ab, int i, int kb) {
    int lo = ab.band_past ? i - (ab.band_past - 1) - kb : 0;
    int hi = ab.band_future ? i + (ab.band_future - 1) - kb : 63;
    lo = lo < 0 ? 0 : lo;
    hi = hi > 63 ? 63 : hi;
    return lo > hi ? 0ull : (~0ull >> (63 - hi)) & (~0ull << lo);
}
// the 64-row blocks at q0 (queries) and k0 (keys) hold a pair the band lets through (the long-dialogue kernels skip the others)
__host__ __device__ inline bool m2f_attn_band_blocks_meet(const AttnBatch& ab, int q0, int k0) {
    return (!ab.band_past || k0 + 63 >= q0 - (ab.band_past - 1)) && (!ab.band_future || k0 <= q0 + 63 + (ab.band_future - 1));
}
int m2f_attn_shadow_only_bits(const AttnBatch& ab, int pi, bool bwd);     // host: operands this launch stages from bf16 shadows only
hipError_t m2f_launch_attn_fwd(AttnBatch& ab, hipStream_t stream);
// Long-sequence forward (S unbounded, hd <= 128): token-level self-attention of the in-loop text encoder (inference).
// q/k/v rows are token-major (token t = b*S + i), head h in columns [h*hd, (h+1)*hd); key_pad [B, S] (1 = padded, nullable).
hipError_t m2f_launch_attn_long_fwd_bf16(const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v, int ldv,
                                         const uint8_t* key_pad, uint16_t* out16, float* out32, uint8_t* out8, float out8_scale, int ldo,
                                         int B, int S, int H, int hd, hipStream_t stream);
hipError_t m2f_launch_attn_long_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                    const uint8_t* key_pad, float* out, int ldo, int B, int S, int H, int hd, ShadowMap sh,
                                    hipStream_t stream);
hipError_t m2f_launch_attn_bwd(AttnBatch& ab, hipStream_t stream);
size_t m2f_attn_probs_elems(int B, int H, int L);
// Long-dialogue forms (attention_dlong.hip): the same AttnBatch contract - packed (cu) or padded (key_pad) - for 1 <= L <= 512,
// one workgroup per 64-row block of a (dialogue, head).  Forward writes P^T to pr[i].probs as above; the backward runs two
// kernels (dK / dV per key block, dQ per query block).  The plans launch them for L > 64; B * H * L * L must stay below 2^32
// (the dropout keep index is 32-bit).
#define M2F_ATTN_DLONG_MAX_L 512
bool m2f_attn_dlong_index_ok(int B, int H, int L);
hipError_t m2f_launch_attn_dlong_fwd(AttnBatch& ab, hipStream_t stream);
hipError_t m2f_launch_attn_dlong_bwd(AttnBatch& ab, hipStream_t stream);

// Attention maps (attention_weights.hip): the saved P^T of up to 64 sites -> torch's need_weights layouts, ONE launch.  Site i: probs as
// the forward launches above leave it ([B*H, Lp, Lp], P^T, pre-dropout), out = [B, H, L, L] (per_head) or [B, L, L] (the sequential fp32
// sum over h = 0 .. H - 1, times inv_h = 1.0f / H computed on the host).  Element (b, [h,] i, j) is READ from probs only if i and j lie
// inside the dialogue (cu: its cu[b+1] - cu[b] rows; key_pad: L), key j is not padded and the band (the two compares of
// m2f_attn_band_bits, band_past / band_future stored + 1 as in AttnBatch) admits (i, j); every other element is written as 0 - the
// long-dialogue forward leaves band-hidden block pairs and the tile rows behind a short dialogue as they were.
#define M2F_ATTN_WEIGHTS_MAX_SITES 64
struct AttnWeightsSite {
    const float* probs;
    float* out;
    int H;
    float inv_h;
};
struct AttnWeightsBatch {
    int sb[M2F_ATTN_WEIGHTS_MAX_SITES];      // first workgroup of site i (INT_MAX for unused slots); filled by the launcher
    AttnWeightsSite site[M2F_ATTN_WEIGHTS_MAX_SITES];
    int count;
    int B, L;
    int per_head;
    int band_past, band_future;              // stored + 1, 0 = unlimited (m2f_attn_weights_set_band)
    int vec;                                 // filled by the launcher: 16-byte stores (L % 4 == 0, every out 16-byte aligned)
    const uint8_t* key_pad;                  // [B, L], 1 = padded key (nullable: every key valid)
    const int* cu;                           // packed layout (nullable): dialogue b holds cu[b+1] - cu[b] utterances; key_pad unused
};
inline void m2f_attn_weights_set_band(AttnWeightsBatch& wb, int past, int future) {
    AttnBatch ab{};
    m2f_attn_set_band(ab, past, future);
    wb.band_past = ab.band_past; wb.band_future = ab.band_future;
}
hipError_t m2f_launch_attn_weights(AttnWeightsBatch& wb, hipStream_t stream);
// ROWS mode, for the rows a stream's weights-emitting step stores: site i's probs = [B][H][L] (B = stream slots, L = capacity, already
// in key order) -> out [B][H][L] (per_head: a copy) or [B][L] by the same head-average rule.  key_pad / cu / the band are not read:
// the step kernel wrote every element.
hipError_t m2f_launch_attn_weight_rows(AttnWeightsBatch& wb, hipStream_t stream);

// Streaming attention (attention_stream.hip): one new utterance per stream slot against the slot's cached K / V rows.  q / k / v: the
// new rows [S, H*hd] (fp32, column slices with a leading dimension, as AttnProblem carries them); kcache / vcache: the site's caches,
// [S][H][C][pad4(hd)] fp32 or [S][H][C][pad8(hd)] bf16 (16-byte aligned).  len[s] = utterances cached so far (read, not advanced),
// active[s] = 0: zero output row, nothing else touched.  ring: the new row goes to len % C and min(len + 1, C) rows are live (a window
// of C - 1 past utterances); otherwise to row len, and a slot with len >= C is treated as inactive (the host refuses it first).
#define M2F_ATTN_STREAM_MAX_C 512
struct AttnStreamProblem {
    const float* q; const float* k; const float* v;
    int ldq, ldk, ldv;
    float* out; int ldo;
    void* kcache; void* vcache;
    int H, hd;
    int block_begin;                                   // filled by the launcher
};
struct AttnStreamBatch {
    int bb[M2F_ATTN_MAX_PROBLEMS];      // block_begin of problem i (INT_MAX for unused slots)
    AttnStreamProblem pr[M2F_ATTN_MAX_PROBLEMS];
    int count;
    int S, C, ring, bf16;      // bf16: caches hold bf16 (K / V rounded once on the way in), q is rounded where it enters the product
    const int* len;            // device int32 [S]
    const uint8_t* active;     // device uint8 [S]
    ShadowMap sh;              // out also written as bf16
    float bias_gain;           // distance-decay bias (m2f_attn_bias_slope): the gain, 0 = off; the new utterance is at distance 0
    // Speaker heads (m2f_attn_speaker_class; (0, 0) = off).  spk_cache: device uint8 [S][C], the speaker id of the utterance in LOGICAL
    // cache row j of slot s (the row index the dense addressing uses, the one a page table maps: dense on a paged stream too), ONE
    // array per stream shared by every site; the attention launches only read it, and never the row the new utterance takes.
    // spk_new: the ids of the new utterances - [S] (step) or [S][T] (chunk).  m2f_launch_stream_advance_speakers[_n] stores them
    // behind the last attention launch of the step / the prefill call.
    const uint8_t* spk_cache;
    const uint8_t* spk_new;
    uint8_t spk_same, spk_other;
};
// host: what a stream launch with speaker heads needs (the launchers refuse the others before anything is launched)
inline bool m2f_attn_stream_speakers_ok(const AttnStreamBatch& ab) {
    if (!(ab.spk_same | ab.spk_other)) return true;
    if (!ab.spk_cache || !ab.spk_new) return false;
    for (int i = 0; i < ab.count && i < M2F_ATTN_MAX_PROBLEMS; ++i)
        if ((int)ab.spk_same + (int)ab.spk_other > ab.pr[i].H) return false;
    return true;
}
// ... and the launches that close a step / a prefill call of a stream with speaker heads: the new ids into the cache rows the new
// utterances took (ring: row u % C - the byte of the utterance that just left the window), then len += what the plain advance adds.
// Plain byte stores, one thread per slot; stream-ordered behind the attention launches that read the old row set.
hipError_t m2f_launch_stream_advance_speakers(int* len, const uint8_t* active, int S, uint8_t* spk_cache, const uint8_t* spk_new, int C,
                                              int ring, hipStream_t stream);
hipError_t m2f_launch_stream_advance_speakers_n(int* len, const int* n_new, int S, int T, uint8_t* spk_cache, const uint8_t* spk_new, int C,
                                                int ring, hipStream_t stream);
size_t m2f_attn_stream_cache_elems(int S, int H, int hd, int C, int bf16);     // elements (fp32 or bf16) of ONE cache (K or V) of a site
hipError_t m2f_launch_stream_advance(int* len, const uint8_t* active, int S, hipStream_t stream);      // len[s] += active[s]
hipError_t m2f_launch_stream_reset(int* len, const uint8_t* mask, int S, hipStream_t stream);          // len[s] = 0 where mask[s] (null: all)
// Chunk form (attention_stream_chunk.hip): slot s takes n_new[s] (0 .. T, T <= 64; device int32 [S]) new utterances - rows s*T + t of
// q / k / v / out - in one launch; what n_new[s] launches of the kernel above give, row by row.  ab.active is not read.  A slot with
// n_new == 0, or a plain cache that the chunk would overfill (len + n_new > C), gets zero output rows and keeps its cache; output rows
// t >= n_new[s] are zeros, their input rows are never read.  len is not advanced: m2f_launch_stream_advance_n adds the clamped n_new.
#define M2F_ATTN_STREAM_MAX_CHUNK 64
hipError_t m2f_launch_stream_advance_n(int* len, const int* n_new, int S, int T, hipStream_t stream);   // len[s] += min(max(n_new[s], 0), T)
// Paged addressing: kcache / vcache of a problem are the site's page POOLS, [n_pages][H][R][pad(hd)] (rows padded and aligned as the
// dense caches'), and logical cache row j of slot s - the row the dense addressing calls j - is row j % R of page table[s][j / R].
// Each streaming kernel is ONE body with two addressings (a template flag): a launch without a paging runs it over per-slot caches,
// a launch with one over pools, and the two give the same bits.  The paging travels as a kernel argument of its own, beside the
// batch.  Only the table entries of pages that hold a live row or take a new one are read; ids are clamped to the pool.
struct AttnStreamPaging {
    const int* table;          // device int32 [S][tw]
    int tw;                    // entries per slot: ceil(C / R)
    int R, lgR;                // rows per page, 16 / 32 / 64 (lgR: filled by the launcher, in its own copy)
    int n_pages;               // pages of every pool
};
size_t m2f_attn_stream_pool_elems(int n_pages, int H, int hd, int R, int bf16);        // elements (fp32 or bf16) of ONE pool (K or V) of a site
bool m2f_attn_stream_paging_ok(const AttnStreamBatch& ab, AttnStreamPaging& pg);       // R, table, tw against ab.C; fills lgR
// The launches; paging == nullptr: dense caches.  Both refuse (hipErrorInvalidValue, nothing launched) what m2f_attn_stream_prepare
// refuses - a bad count, S, C > 512, hd > 128, a null or misaligned cache / pool, a paging that is not ok - and fill block_begin / bb[].
int m2f_attn_stream_prepare(AttnStreamBatch& ab, AttnStreamPaging* pg, int* maxW);     // -> workgroups or -1; maxW: widest pad16(hd)
// weights != nullptr: the weights-emitting form of the step kernel - problem i also stores its rows of probabilities to weights->w[i],
// fp32 [S][H][C], column t = the t-th oldest live utterance of the slot (zeros behind the live count and for inactive slots).  Like the
// paging it travels as a kernel argument of its own: a launch without it runs the kernels it always ran.
struct AttnStreamWeights { float* w[M2F_ATTN_MAX_PROBLEMS]; };
hipError_t m2f_launch_attn_stream(AttnStreamBatch& ab, const AttnStreamPaging* paging, hipStream_t stream, const AttnStreamWeights* weights = nullptr);
hipError_t m2f_launch_attn_stream_chunk(AttnStreamBatch& ab, const AttnStreamPaging* paging, int T, const int* n_new, hipStream_t stream);
// Snapshot / restore of those caches (stream_cache.hip has the packed layout): entry e of n_entries = the min(lengths[e], C) live
// physical rows of slot slots[e], every listed site, K then V, packed at row row_offsets[e].  One launch for all sites and entries
// (slices of 65,535 entries); the kernels move 16-byte vectors, so a site is described by `vpr` = vectors per padded row and the
// element type never enters.  kcache / vcache: the site's caches, or (with a paging) its pools.  scatter: packed -> caches, and
// len[slot] = lengths[e]; otherwise caches -> packed.  An entry that is out of range (slot, length, offset, rows past packed_vecs)
// is skipped whole by the kernel.
#define M2F_STREAM_CACHE_MAX_SITES 64
struct StreamCacheSite {
    void* kcache; void* vcache;
    int H;
    int vpr;                   // 16-byte vectors per padded row: m2f_stream_cache_row_vecs(hd, bf16)
    int colv;                  // vectors of one packed row that belong to the sites before this one
    int pad_;
};
struct StreamCacheBatch {
    int sb[M2F_STREAM_CACHE_MAX_SITES];      // first segment (blockIdx.x) of site i (INT_MAX for unused slots); filled by the launcher
    StreamCacheSite site[M2F_STREAM_CACHE_MAX_SITES];
    int count;
    int S, C;
    int rowv;                  // vectors of one packed row, all sites of the FORMAT (>= what the listed sites cover)
    int n_entries, e0;         // e0: first entry of the launch (filled by the launcher)
    const int* slots;          // device int32 [n_entries]
    const int* lengths;        // device int32 [n_entries]: utterances of the entry (a ring: the unwrapped count)
    const int64_t* row_offsets;     // device int64 [n_entries]: first packed row of the entry
    void* packed;              // 16-byte aligned
    int64_t packed_vecs;       // vectors the packed buffer holds
    int* len;                  // scatter: device int32 [S], the plan's counters
};
int m2f_stream_cache_row_vecs(int hd, int bf16);
hipError_t m2f_launch_stream_cache(StreamCacheBatch& cb, const AttnStreamPaging* paging, int scatter, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// Row-wise kernels
// ------------------------------------------------------------------------------------------------
struct LnProblem {
    // forward: y = LN(x)*gamma + beta ; out = (res ? res : 0) + y ; optional dropout(out)
    const float* x; const float* gamma; const float* beta; const float* res;
    float* out; float* stats;          // stats [T, 2] = (mean, rstd)
    int d;
    int ld;                            // row stride of x / res / out / dy / extra / dx / dx_masked (0 = d)
    uint32_t drop_site;
    // backward: dx = LNbwd(dy) (+ extra) ; optional second output dx_masked = LNbwd(dy) * keep(site2)/(1-p)
    const float* dy; const float* extra;
    float* dx; float* dx_masked;
    float* partial;                    // [n_row_blocks, 2, d] partial (dgamma, dbeta)
    uint32_t drop_site2;
    int block_begin;
    // bf16 mode, set by plan_build.hip::mark_unread_fp32 - copies nobody reads: 1 = dx_masked as fp32 (only GEMMs stage it, from its
    // shadow), 2 = dx as bf16 (it is only a residual term / a LayerNorm input)
    uint32_t skip;
};
#define M2F_LN_MAX_PROBLEMS 4
struct LnBatch {
    int bb[M2F_LN_MAX_PROBLEMS];        // block_begin of problem i (INT_MAX for unused slots)
    LnProblem pr[M2F_LN_MAX_PROBLEMS];
    int count;
    int T;
    float eps;
    const uint32_t* rng; uint32_t drop_thresh; float drop_scale;
    ShadowMap sh;                      // out (fwd) / dx, dx_masked (bwd) also written as bf16
    int pre_stats;                     // forward, diagnostic (tools/ln_stats_ab.py): 1 = mean / rstd are READ from `stats` instead of computed (what a LayerNorm
                                       // whose statistics came out of the preceding GEMM's epilogue would cost)
    uint8_t* out8; float out8_scale;   // forward, problem 0 only (nullable): out ALSO as OCP e4m3 bytes of value * out8_scale, saturating, row stride d
                                       // (the operand the text encoder's fp8 GEMMs stage: no quantise pass; d % 4 == 0)
};
#define M2F_LN_ROWS_PER_BLOCK 4
hipError_t m2f_launch_ln_fwd(LnBatch& lb, hipStream_t stream);
hipError_t m2f_launch_ln_bwd(LnBatch& lb, hipStream_t stream);
static inline int m2f_ln_row_blocks(int T) { return (T + M2F_LN_ROWS_PER_BLOCK - 1) / M2F_LN_ROWS_PER_BLOCK; }

// dgamma/dbeta = sum over row blocks of the partials, for many LayerNorms in one launch.
struct LnReduceItem { const float* partial; float* dgamma; float* dbeta; int d; int nblk; };
#define M2F_LNRED_MAX_ITEMS 32
struct LnReduceBatch { LnReduceItem it[M2F_LNRED_MAX_ITEMS]; int count; };
// accumulate != 0: dgamma / dbeta = old + the reduced sum (the accumulate form of the backward, m2f_plan_accumulate_grads)
hipError_t m2f_launch_ln_param_reduce(const LnReduceBatch& rb, hipStream_t stream, int accumulate = 0);

// Criterion of src/train.py:48-50 on logits [T, C] (C <= 16): CrossEntropyLoss(ignore_index=-1,
// label_smoothing, optional class weights).  Per token it writes the loss numerator / denominator
// terms and the UNNORMALISED gradient d(sum of numerators)/dlogits.  ONE struct and ONE launch for the plain criterion and its
// three extensions; m2f_launch_ce picks the kernel from which optional pointers are set.  Below, ce / g = the plain numerator and
// gradient of a row with a valid label y; rows with an invalid label write zeros whatever their teacher or twin row holds.
//
// Distillation (teacher, hyper).  q = softmax(z / tau), p = softmax(teacher / tau):
//   numerator   = (1 - alpha) * ce + alpha * tau^2 * w_y * KL(p || q)                     denominator = w_y, as the plain one
//   dlogits     = (1 - alpha) * g  + alpha * tau * w_y * (q - p)                          (unnormalised, as the plain one)
// alpha and tau are READ FROM THE DEVICE (hyper[0], hyper[1]): a captured step replays while a schedule changes them.
// alpha = 0 gives the plain bits.
//
// Focal (gamma; Lin et al. 2017): the hard-label term scaled by (1 - p_y)^gamma.  omp = sum of p_c over c != y, the other classes'
// probabilities ADDED, never 1 - p_y:
//   numerator   = omp^gamma * ce
//   dlogits_c   = omp^gamma * g_c + ce * gamma * omp^gamma * p_y * r_c      r_c = p_c / omp for c != y, r_y = -1
// (= ce * gamma * omp^(gamma - 1) * p_y * d_c with d_c = p_c, d_y = -omp; the quotient form keeps every factor <= 1, so no gamma in
// (0, 1) overflows at a tiny omp).  With a teacher the factor scales the hard-label term of the distillation form only:
// numerator = (1 - alpha) * omp^gamma * ce + alpha * tau^2 * w_y * KL, the teacher's gradient term unchanged.
// gamma is READ FROM THE DEVICE (gamma[0], in [0, 8]): a captured step replays while a schedule changes it.  gamma == 0 selects factor 1
// and slope 0: the plain bits (with a teacher the distillation's).  omp == 0 selects factor and slope 0 for gamma > 0.
//
// R-Drop (partner, alpha, kl_terms; Liang et al. 2021): every token row r is coupled to its twin t(r) = partner[r] - the same utterance
// under another dropout mask, a row of the SAME logits buffer.  p = softmax(z_r), q = softmax(z_t(r)):
//   s           = 0.5 * sum_c (p_c - q_c) * (logp_c - logq_c)      = 0.5 * (KL(p || q) + KL(q || p)), the same bits on both rows of a pair
//   numerator   = ce + alpha * w_y * s
//   dlogits_c   = g_c + alpha * w_y * (p_c * ((logp_c - logq_c) - KL(p || q)) + (p_c - q_c))
// (the twin's row carries the mirror term, so the pair's two gradients are the gradient of w_y * (s_r + s_t(r)) = 2 w_y s.)  kl_terms[r] =
// w_y * s, WITHOUT alpha: m2f_launch_rdrop_kl_reduce sums it in the finalize launch's order.  logp / logq come from the log-softmax,
// never from log(p): a probability that underflows contributes 0 * finite = 0.  alpha is READ FROM THE DEVICE (alpha[0] >= 0): a captured
// step replays while a warm-up changes it; alpha == 0 gives the plain bits.  partner[r] outside [0, T): no twin, the plain term.
struct CeArgs {
    const float* logits; int T, C;
    const int64_t* labels;                 // [T], ignore_index = -1
    const float* class_w;                  // [C] or null
    float label_smoothing;
    float* loss_terms;                     // [T, 2] (numerator, denominator)
    float* dlogits;                        // [T, C]
    // ---- optional: what is set selects the kernel ----
    const float* teacher = nullptr;        // [T, C] teacher logits, token rows as logits: distillation (with gamma: its focal form)
    const float* hyper = nullptr;          // device float [2]: alpha in [0, 1], tau > 0; read only with a teacher
    const float* gamma = nullptr;          // device float [1]: focal
    const int32_t* partner = nullptr;      // [T]: the twin of every token row, or -1: R-Drop (no teacher, no gamma)
    const float* alpha = nullptr;          // device float [1], with partner
    float* kl_terms = nullptr;             // [T]: w_y * s, with partner
};
// partner: R-Drop; else gamma: focal (with or without a teacher); else teacher: distillation; else the plain kernel.
// hipErrorInvalidValue for a combination without a kernel: partner with teacher or gamma, teacher without hyper, partner without
// alpha or kl_terms.
hipError_t m2f_launch_ce(const CeArgs& a, hipStream_t stream);
// loss_out[3] = (accumulate: +=) sum of kl_terms, summed in m2f_launch_loss_finalize's order (thread-strided, wave sum, (s0 + s1) + (s2 + s3))
hipError_t m2f_launch_rdrop_kl_reduce(const float* kl_terms, int T, float* loss_out, hipStream_t stream, int accumulate = 0);
// Supervised contrastive criterion over feature rows (supcon.hip holds the definition: V, z, s, l_i, c_i, dz, dh).  Exact fp32 on
// v_mfma_f32_16x16x4_f32 whatever the plan's precision.  lambda and tau are READ FROM THE DEVICE (hyper[0] >= 0, hyper[1] > 0): a
// captured step replays while a schedule changes them; lambda == 0 gives dfeat = 0 and adds 0 to every numerator.
//   row_terms[i] = (lse_i, n_i, l_i, w_{y_i} l_i)        zeros outside V; l = 0 for a row of V without a positive (its lse is still given)
//   dfeat[i, :]  = lambda-weighted d (sum_i w_{y_i} l_i) / d h_i, unnormalised (no 1 / den), zeros outside V
//   loss_terms   (nullable) [N, 2]: the numerator of row i += lambda * w_{y_i} * l_i; the denominator is untouched
struct SupconArgs {
    const float* feat; int N, D, ld;       // [N, D], row stride ld
    const int64_t* labels; int C;          // [N], a label outside [0, C) = not in V
    const float* class_w;                  // [C] or null
    const float* hyper;                    // device float [2]: lambda, tau
    float* ws;                             // m2f_supcon_ws_floats(N, D) floats, 16-byte aligned
    float* row_terms;                      // [N, 4], 16-byte aligned
    float* dfeat; int ldd;                 // [N, D], row stride ldd
    float* loss_terms = nullptr;
};
size_t m2f_supcon_ws_floats(int N, int D);
hipError_t m2f_launch_supcon(const SupconArgs& a, hipStream_t stream);
// loss_out[3] = (accumulate: +=) sum of row_terms' w l in m2f_launch_loss_finalize's order; scale[0] = the factor that launch multiplies
// dlogits by for the same loss_terms (1 / den, the same bits; 1 without normalise)
hipError_t m2f_launch_supcon_tail(const float* row_terms, const float* loss_terms, int T, float* loss_out, float* scale, int normalise,
                                  hipStream_t stream, int accumulate = 0);
// dh[i, :] += (h[i, :] > 0 ? gate_scale : 0) * scale[0] * dfeat[i, :] over [T, d] buffers of one row stride; write16: dh's bf16 shadow too
hipError_t m2f_launch_supcon_add(float* dh, const float* h, const float* dfeat, const float* scale, int T, int d, int ld, float gate_scale,
                                 int write16, ShadowMap sh, hipStream_t stream);
// Auxiliary label head over feature rows (aux_head.hip holds the definition: u = W h + b scored against its own labels, weighted by the
// PRIMARY label's class weight).  Exact fp32 whatever the plan's precision.  lambda and eps_a are READ FROM THE DEVICE (hyper[0] >= 0,
// 0 <= hyper[1] < 1): a captured step replays while a schedule changes them; lambda == 0 adds 0 to every numerator and gradient.
//   aux_logits[i, c] = u_ic (every row)      row_term[i] = w_{y_i} a_i      g[i, c] = w_{y_i} d a_i / d u_ic   (zeros on an ignored row)
//   loss_terms   (nullable) [N, 2]: the numerator of row i += lambda * w_{y_i} * a_i; the denominator is untouched
struct AuxHeadArgs {
    const float* feat; int N, D, ld;       // [N, D], row stride ld (a multiple of 4, rows 16-byte aligned), D <= 1,024
    const float* params; int A;            // [W (A x D) | b (A)], 16-byte aligned, 2 <= A <= 16
    const int64_t* labels; int C;          // [N] primary labels, a label outside [0, C) = ignored row
    const float* class_w;                  // [C] or null
    const int64_t* aux_labels;             // [N], a label outside [0, A) = ignored row; null: the logits alone (labels, hyper, g, row_term unused)
    const float* hyper;                    // device float [2]: lambda, eps_a
    float* aux_logits; int ldu;            // [N, A], row stride ldu
    float* g;                              // [N, 16]
    float* row_term;                       // [N]
    float* loss_terms = nullptr;
};
// g [N, 16] | row_term [N] | the parameter gradient's partials, one per 16 rows
size_t m2f_aux_head_ws_floats(int N, int D, int A);
hipError_t m2f_launch_aux_rows(const AuxHeadArgs& a, hipStream_t stream);
// loss_out[3] = (accumulate: +=) sum of row_term in m2f_launch_loss_finalize's order; scale[0] = the factor that launch multiplies dlogits
// by for the same loss_terms (1 / den, the same bits; 1 without normalise)
hipError_t m2f_launch_aux_tail(const float* row_term, const float* loss_terms, int T, float* loss_out, float* scale, int normalise,
                               hipStream_t stream, int accumulate = 0);
// dh[i, :] = (add: dh[i, :] +) gate * scale[0] * hyper[0] * sum_c g[i, c] W[c, :], gate = (h[i, :] > 0 ? gate_scale : 0) or (h null) 1;
// scale / hyper null = 1; write16: dh's bf16 shadow too.  g: [N, A] with row stride ldg
hipError_t m2f_launch_aux_join(float* dh, int ldd, const float* h, int ld, const float* g, int ldg, const float* params, int A, int N, int D,
                               const float* scale, const float* hyper, float gate_scale, int add, int write16, ShadowMap sh, hipStream_t stream);
// grad [A D + A] = scale[0] * hyper[0] * [g^T h | sum_i g[i, :]] (overwritten); part: the third share of m2f_aux_head_ws_floats
hipError_t m2f_launch_aux_param_grad(const float* h, int ld, const float* g, int ldg, int A, int N, int D, float* part, const float* scale,
                                     const float* hyper, float* grad, hipStream_t stream);
// Linear-chain CRF over a dialogue's labels (crf.hip).  params: float [C*C + 2C] = [transitions row-major C x C | start C | end C], 2 <= C <= 16.
// Dialogue b owns token rows cu_seqlens[b] .. cu_seqlens[b+1]-1 (packed and long-dialogue plans) or, cu_seqlens null, b*L .. b*L+L-1
// (padded and bucket-padded plans).  The CHAIN of a dialogue is its rows with a label in [0, C), in row order (a -1 in the middle links
// its neighbours; the logits of an unlabelled row are never read).  With t_1 < ... < t_n the chain rows, e the logits, y the labels:
//   score(y) = start[y_1] + sum_k e[t_k, y_k] + sum_{k>=2} transitions[y_{k-1}, y_k] + end[y_n]     logZ = log sum_paths exp(score)
//   loss_terms: num = logZ - score(y) on the dialogue's first chain row, 0 elsewhere; den = 1 on every chain row (token_mean through
//               m2f_launch_loss_finalize, unchanged)
//   dlogits[t_k, c] = P(y_k = c) - [c == y_k], zeros on every other row (unnormalised: the finalize launch scales it)
//   partial (nullable = frozen parameters): [B][C*C + 2C] per-dialogue d transitions, d start, d end in the layout of params;
//               m2f_launch_crf_grad_reduce adds them in dialogue order and, normalise != 0, divides by loss_out[1]
// A dialogue without a chain row contributes zeros everywhere.  ws: float [T * (2C + 2)] (the saved chain rows of the backward sweep).
struct CrfArgs {
    const float* logits; int T, C;         // [T, C]
    const int64_t* labels;                 // [T], -1 = not on the chain
    const float* params;                   // [C*C + 2C]
    const int32_t* cu_seqlens; int B, L;   // [B + 1] or null (then rows b*L + i)
    float* ws;                             // [T * (2C + 2)]
    float* loss_terms;                     // [T, 2]
    float* dlogits;                        // [T, C], or null: the loss only (no backward sweep; the evaluation path) - partial must be null too
    float* partial;                        // [B, C*C + 2C] or null
};
hipError_t m2f_launch_crf_nll(const CrfArgs& a, hipStream_t stream);
hipError_t m2f_launch_crf_grad_reduce(const float* partial, int B, int C, const float* loss_out, int normalise, float* grad,
                                      hipStream_t stream);
// Viterbi over the rows whose mask is 0: pred[t] = the best path's class (-1 off the chain), score[b] = the path's score (0 for a
// dialogue without a chain row).  First-max rule everywhere: the lowest class wins a tie.  ws: int [T * 5] (back pointers).
struct CrfViterbiArgs {
    const float* logits; int T, C;
    const uint8_t* mask;                   // [T], 1 = not on the chain; null: every row of a dialogue is on it
    const float* params;
    const int32_t* cu_seqlens; int B, L;
    int* ws;                               // [T * 5]
    int32_t* pred;                         // [T]
    float* score;                          // [B]
};
hipError_t m2f_launch_crf_viterbi(const CrfViterbiArgs& a, hipStream_t stream);
// Forward filter of the streams: per slot phi = a - logsumexp(a), a = e + logsumexp_i(phi_old[i] + transitions[i, :]), a = start + e for
// the slot's first utterance (count[s] + rows taken so far == 0).  Slot s takes rows s*rows .. s*rows + n_new[s] - 1 of logits in order
// (n_new null: one row; active null: every slot; an inactive slot keeps its phi).  count is read, never written.
struct CrfFilterArgs {
    const float* logits; int S, C, rows;   // [S * rows, C]
    const float* params;
    const int32_t* count;                  // [S]
    const uint8_t* active;                 // [S] or null
    const int32_t* n_new;                  // [S] or null
    float* phi;                            // [S, C], in and out
};
hipError_t m2f_launch_crf_filter(const CrfFilterArgs& a, hipStream_t stream);
// loss_out[0] = num/den, loss_out[1] = den, loss_out[2] = num.  normalise != 0: dlogits *= 1/den
// (single-process mean-over-valid loss); normalise == 0 leaves the sum-gradient for the data-parallel
// path, which divides by the GLOBAL denominator after the all-reduce.
// accumulate != 0: loss_out[1] and loss_out[2] ADD this batch's den and num to what they hold (loss_out[0] is still this batch's num / den)
hipError_t m2f_launch_loss_finalize(const float* loss_terms, int T, int C, float* dlogits, float* loss_out,
                                    int normalise, hipStream_t stream, int accumulate = 0);

// Scoring of one evaluation batch (metrics.hip; src/train.py:245-272, src/test.py:51-74 of the reference): the criterion's loss without
// its gradient, first-max argmax, the C x C confusion matrix, accuracy and weighted F1, ADDED to `record` (M2F_EVAL_RECORD_HEAD
// doubles: loss_sum, acc_sum, f1_sum, n_batches, the last batch's loss / accuracy / F1, one unused; then C x C int64).  Two launches.
#define M2F_EVAL_MAX_C 16
#define M2F_EVAL_MAX_BLOCKS 128
#define M2F_EVAL_RECORD_HEAD 8
struct EvalArgs {
    const float* logits; int T, C;
    const int64_t* labels;                 // [T], -1 = unlabelled (pad and filler rows)
    const float* class_w;                  // [C] or null
    float label_smoothing;
    float* terms;                          // [T, 2] (numerator, denominator), as CeArgs::loss_terms
    int* partial;                          // [m2f_eval_blocks(T)][C * C]: one integer tile per workgroup of the rows launch
    const float* gamma = nullptr;          // device float [1] or null: non-null runs the focal form of the rows launch (the loss of CeArgs::gamma
                                           // without a teacher, no gradient); null: the default form, its bits unchanged
    const int32_t* pred = nullptr;         // [T] or null: non-null runs the prediction form of the rows launch - the labels counted against pred
                                           // (a decoded path, -1 = none) instead of the argmax, `terms` left as the launch in front wrote them
};
static inline int m2f_eval_blocks(int T) { const int b = (T + 255) / 256; return b < M2F_EVAL_MAX_BLOCKS ? b : M2F_EVAL_MAX_BLOCKS; }
hipError_t m2f_launch_eval_scores(const EvalArgs& a, double* record, hipStream_t stream);

// fp32 -> bf16 (round to nearest even) of up to M2F_CAST_MAX_ITEMS 2-D blocks in one launch: dst[r*ldd + c] =
// bf16(src[r*lds + c]) for c < cols (pad columns of dst are left untouched = zero).
struct CastItem { const float* src; uint16_t* dst; int rows, cols, lds, ldd; uint16_t* dst_t; int ldd_t; };   // dst_t: transposed copy [cols][rows] (nullable)
#define M2F_CAST_MAX_ITEMS 48
struct CastBatch { CastItem it[M2F_CAST_MAX_ITEMS]; int count; };
hipError_t m2f_launch_cast(const CastBatch& cb, hipStream_t stream);


// Dialogue batcher (replaces Dataset.__getitem__ + collate_fn, reference src/dataset.py:32-89, on the device): token slot t
// takes row rows[t] of the two device-resident embedding tables (rows[t] < 0: padded slot -> zeros, label -1, key_pad 1).
struct GatherArgs {
    const float* text_table; const float* audio_table; const int64_t* label_table;
    const int32_t* rows;
    int T, d_text, d_audio, ld_text, ld_audio;
    float* text_out; float* audio_out; uint8_t* key_pad; int64_t* labels;
};
hipError_t m2f_launch_gather(const GatherArgs& a, hipStream_t stream);

// RoBERTa embeddings + LayerNorm (in-loop text encoder): out[t] = LN(word[ids[t]] + pos[pos_ids[t]] + type0)
hipError_t m2f_launch_embed_ln(const int64_t* ids, const int64_t* pos_ids, const float* word, const float* pos, const float* type0,
                               const float* gamma, const float* beta, float eps, float* out, int ld, int T, int d, ShadowMap sh,
                               hipStream_t stream);

// dst[i] = e4m3(clamp(src[i] * scale, +-448)) for n values (n % 4 == 0): operand quantisation of the fp8 GEMMs
hipError_t m2f_launch_quant_fp8(const float* src, uint8_t* dst, int64_t n, float scale, hipStream_t stream);

// in-place: x[t, c] *= keep(site, t*d + c) / (1 - p)
// (x2 != null: a second buffer of the same shape with its own site, same launch)
hipError_t m2f_launch_dropout_inplace2(float* x, float* x2, int T, int d, int ld, uint32_t site, uint32_t site2, const uint32_t* rng,
                                       uint32_t thresh, float scale, ShadowMap sh, hipStream_t stream);
hipError_t m2f_launch_dropout_inplace(float* x, int T, int d, int ld, uint32_t site, const uint32_t* rng,
                                      uint32_t thresh, float scale, ShadowMap sh, hipStream_t stream);
// rng.step += 1 (device side, graph-replay safe)
hipError_t m2f_launch_rng_advance(uint32_t* rng, hipStream_t stream);

// Fused Adam with coupled L2 (torch.optim.Adam semantics, src/train.py:56) over the flat buffers.
// grad_scale_ptr (device, may be null): gradients are multiplied by 1 / *grad_scale_ptr first (the
// global valid-utterance denominator under data parallelism).
// g_is_bf16: g points at bf16 gradients (data-parallel bf16 exchange) instead of fp32.
// ema (device, may be null; here and in the three forms below): the exponential moving average of the parameters, same indexing as p -
// after the update e <- (ema_w == 1) ? p : fma(ema_w, p - e, e), ema_w = (float)(1 - decay); null: the kernel without the stream.
hipError_t m2f_launch_adam(float* p, const void* g, int g_is_bf16, float* m, float* v, int64_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                           float* ema, float ema_w, hipStream_t stream);

// Fused Adam + parameter-shadow refresh (bf16 mode, single process): the same update as m2f_launch_adam, walked matrix by matrix
// in 64x64 tiles so that the kernel that has the new fp32 parameter in registers also writes its bf16 shadows - W [rows][pad8(cols)]
// and W^T [cols][pad8(rows)] through an LDS tile - which the forward / input-gradient GEMMs stage from.  The cast launches at
// the head of the forward (8 B of traffic per parameter, 2 x 87 us at C3) disappear.  Items live in device memory:
// rows > 0: a 2-D parameter (tiles of 64 x 64); rows == 0: `cols` consecutive elements (1-D parameters incl. their pads; tiles
// of 4096 elements).
struct AdamItem { long long off, soff, soff_t; int rows, cols, tile_begin, tiles_c; };
#define M2F_ADAM_MAX_ITEMS 1024
hipError_t m2f_launch_adam_shadowed(float* p, const void* g, int g_is_bf16, float* m, float* v, uint16_t* shadow, const AdamItem* items,
                                    const int* tile_begin, int n_items, int tile_first, int total_tiles, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                                    float* ema, float ema_w, hipStream_t stream);

hipError_t m2f_launch_cast_items(const float* src, uint16_t* dst, const AdamItem* items, const int* tile_begin, int n_items, int total_tiles, hipStream_t stream);
hipError_t m2f_launch_adam_hyper(float* hyper_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int step, hipStream_t stream);
hipError_t m2f_launch_adam_shadowed_dev(float* p, const float* g, float* m, float* v, uint16_t* shadow, const AdamItem* items, const int* tile_begin,
                                        int n_items, int total_tiles, const float* hyper_dev, const float* grad_scale_ptr, hipStream_t stream);

// Parameter groups (optim.FusedAdam(params=[...]) / FusedAdamW; torch.optim.Adam / AdamW with several param_groups).  The hyper table
// holds one row of 8 floats per group in device memory: lr / bc1, beta1, beta2, eps, coupled weight decay, 1 / sqrt(bc2), decay, spare -
// decay = 1 - lr * weight_decay for a decoupled group (whose coupled weight decay is 0), 1.0f otherwise.  rows_host: n_groups x 8 floats,
// passed to the refresh kernel by value.  The shadow-writing form walks items[] (the tensors some group owns, re-tiled; item_group[] runs
// parallel to it); the flat form walks slices of at most M2F_PARAM_SLICE elements of one owned tensor (fp32 mode: no shadows).
// ParamSlice: the one slice of the per-tensor kernels (adam.hip and sam.hip through param_walk.h; gradnorm.hip, tensor_stats.hip) - at most M2F_PARAM_SLICE
// consecutive elements of ONE parameter tensor (`off`: its first element in the flat buffer; only the last slice of a tensor is short),
// cut by the host from the parameter map (param_tables.hip), so the alignment pads between tensors belong to no slice.  tag: the owning
// group for the grouped Adam and exchange kernels, the tensor's index for the statistics kernels; the norm kernel does not read it.
#define M2F_PARAM_SLICE 8192     // (M2F_ADAM_MAX_GROUPS: include/m2fnet_hip.h)
struct ParamSlice { long long off; int n; int tag; };
hipError_t m2f_launch_adam_hyper_groups(float* table_dev, const float* rows_host, int n_groups, hipStream_t stream);
hipError_t m2f_launch_adam_shadowed_grouped(float* p, const void* g, int g_is_bf16, float* m, float* v, uint16_t* shadow, const AdamItem* items,
                                            const int* tile_begin, const int* item_group, int n_items, int tile_first, int total_tiles,
                                            const float* hyper_table, const float* grad_scale_ptr, float* ema, float ema_w,
                                            hipStream_t stream);
hipError_t m2f_launch_adam_slices(float* p, const void* g, int g_is_bf16, float* m, float* v, const ParamSlice* slices, int s0, int s1,
                                  const float* hyper_table, const float* grad_scale_ptr, float* ema, float ema_w, hipStream_t stream);
// p[i] <-> ema[i] over the slices [s0, s1) (whole owned tensors; pads and unowned tensors are in no slice)
hipError_t m2f_launch_ema_exchange(float* p, float* ema, const ParamSlice* slices, int s0, int s1, hipStream_t stream);

// Global gradient norm + clip record (gradnorm.hip), over the slices of every tensor (ParamSlice above; the same device array the
// statistics walk).  Stage 1 writes partial[s], one float64 sum of squares per slice of [s0, s1)
// (grid <= 0: min(2048, slices) workgroups; the value of partial[s] does not depend on the grid); the finalize launch sums
// partial[0, n) in index order and writes record = (norm, coef, divisor, sqrt(sum of squares)) as fp32 - see the kernel.
hipError_t m2f_launch_grad_sumsq(const void* g, int g_is_bf16, const ParamSlice* slices, int s0, int s1, double* partial, int grid,
                                 int nontemporal, hipStream_t stream);
hipError_t m2f_launch_grad_norm_finalize(const double* partial, int n, const float* den_ptr, double max_norm, float* record,
                                         hipStream_t stream);

// Sharpness-aware minimisation (sam.hip).  The finalize launch sums partial[0, n) as the clip finalize does and writes record =
// (norm / den, c, den, sqrt(sum of squares)), c = rho / (norm / den + 1e-12) / den; the perturb launches read c = record[1] when they run:
// saved <- w, w <- fma(c, g, w) over parameter elements only.  Shadowed form: items as m2f_launch_adam_shadowed walks them, except that a
// 1-D item's `cols` is the tensor's own element count (no pad), tile_begin from 0; it writes the W / W^T bf16 shadows of w' as that kernel
// lays them out.  Flat form and restore (w <- saved): every tensor's ParamSlices.
hipError_t m2f_launch_sam_finalize(const double* partial, int n, const float* den_ptr, double rho, float* record, hipStream_t stream);
hipError_t m2f_launch_sam_perturb_shadowed(float* p, const void* g, int g_is_bf16, float* saved, uint16_t* shadow, const AdamItem* items,
                                           const int* tile_begin, int n_items, int total_tiles, const float* record, hipStream_t stream);
hipError_t m2f_launch_sam_perturb_flat(float* p, const void* g, int g_is_bf16, float* saved, const ParamSlice* slices, int n_slices,
                                       const float* record, hipStream_t stream);
hipError_t m2f_launch_sam_restore(float* p, const float* saved, const ParamSlice* slices, int n_slices, hipStream_t stream);

// Adversarial ascent on one modality's token rows (adversarial.hip has the definition).  Rows of width d, row stride ld (a multiple of 4,
// >= d rounded up to 4; 16-byte aligned buffers); skip[t] != 0: row t is neither read for a norm nor written; hyper = (epsilon, step) on
// the device; g may be null (zero gradient: the projection alone).  batch_norm: the L2 norm over all rows instead of per row - two
// launches, partial = 3 * m2f_adv_slices(T) doubles of scratch (the launcher fills n_slices).
struct AdvArgs {
    const float* x_clean; const float* g; float* delta; float* x; const uint8_t* skip; const float* hyper; double* partial;
    int T, d, ld, n_slices;
};
int m2f_adv_slices(int T);
hipError_t m2f_launch_adv_ascend(const AdvArgs& a, int batch_norm, hipStream_t stream);
// delta[t, c] = scale * (2 * (h >> 8) * 2^-24 - 1) over the rows that are not skipped, h the dropout hash of element t * d + c under `site`
hipError_t m2f_launch_adv_init(float* delta, int T, int d, int ld, const uint8_t* skip, float scale, const uint32_t* rng, uint32_t site,
                               hipStream_t stream);

// Per-tensor statistics and histograms of a flat buffer (tensor_stats.hip).  slices: every tensor's ParamSlices, tag = the index of the slice's
// tensor; tensor_begin[t] = first slice of tensor t, [n_tensors] = n_slices.  Pass 1 writes partial[s] (a slice's finite count is
// n - nan - inf), the finalize launch the record header (M2F_TSTATS_HEADER doubles: den, n_tensors, bins, 0) and one row per tensor
// (M2F_TSTATS_FIELDS doubles - numel, finite, nan, inf, zeros, min, max, sum, sumsq - then `bins` int64 counts, zeroed), pass 2 adds the
// counts.  passes: bit 0 = pass 1 + finalize, bit 1 = pass 2 (which needs the rows of an earlier pass 1).  b (fp32, or null): x = a - b.
struct StatPartial { double sum, sumsq; float mn, mx; int nan, inf, zeros, pad_; };
#define M2F_TSTATS_HEADER 4
#define M2F_TSTATS_FIELDS 9
#define M2F_TSTATS_MAX_BINS 256
hipError_t m2f_launch_tensor_stats(const void* a, int a_is_bf16, const float* b, const ParamSlice* slices, const int* tensor_begin,
                                   int n_slices, int n_tensors, int bins, const float* den_ptr, StatPartial* partial, double* record,
                                   int grid, int nontemporal, int passes, hipStream_t stream);

#ifdef __HIPCC__
// shadow address of a workspace element, or null (no shadows / pointer outside the workspace, e.g. the gradient buffer)
__device__ __forceinline__ uint16_t* m2f_shadow_of(const ShadowMap& sh, const float* p) {
    if (!sh.ws_base) return nullptr;
    const ptrdiff_t i = p - sh.ws_base;
    return (i >= 0 && (size_t)i < sh.ws_floats) ? sh.shadow + i : nullptr;
}
// Speaker heads, the test per score element.  `ks` = the speaker id of key `lane` of a 64-key block, held by that lane;
// m2f_spk_pack4: the ids of keys base .. base + 3 (the four keys of one accumulator register quad), one byte each.
__device__ __forceinline__ uint32_t m2f_spk_pack4(int ks, int base) {
    uint32_t w = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) w |= ((uint32_t)__shfl(ks, base + r, 64) & 255u) << (8 * r);
    return w;
}
// does a query of speaker `mine` under head class `cls` (wave-uniform) see key r of the pack?
__device__ __forceinline__ bool m2f_spk_sees(int cls, uint32_t pack, int r, int mine) {
    const bool eq = ((pack >> (8 * r)) & 255u) == (uint32_t)mine;
    return cls == M2F_SPK_NONE || eq == (cls == M2F_SPK_SAME);
}
#endif

// ------------------------------------------------------------------------------------------------
// wav2vec2 audio encoder front end (audio_conv.hip; wav2vec2.py drives it, conv layers 1.. run on m2f_launch_gemm)
// ------------------------------------------------------------------------------------------------
#define M2F_W2V_CONV0_MAX_TAPS 16
#define M2F_W2V_CONV0_MAX_STRIDE 8
#define M2F_W2V_FEAT_MAX_C 1024
#define M2F_W2V_POS_MAX_TAPS 256
int m2f_w2v_conv0_chunks(int T0);            // partial statistics: 2 floats per (utterance, chunk, channel); stats: 2 per (utterance, channel)
hipError_t m2f_launch_w2v_conv0(const float* wave, int B, int N, const float* w0, int k0, int s0, int C, int T0, int P0, const float* gamma,
                                const float* beta, float eps, float* partial, float* stats, float* out32, uint16_t* out16,
                                hipStream_t stream);
hipError_t m2f_launch_w2v_feat_ln(const float* x, int B, int S, int P, int C, const float* gamma, const float* beta, float eps, float* out32,
                                  uint16_t* out16, hipStream_t stream);
size_t m2f_w2v_pos_conv_lds(int CG, int K, int bf16);
hipError_t m2f_launch_w2v_pos_conv(const float* x, const int* lengths, int B, int S, int d, int groups, int K, const void* w, const float* bias,
                                   float* out, int bf16, hipStream_t stream);
hipError_t m2f_launch_w2v_masked_mean(const float* x, const int* lengths, int B, int S, int d, float* out, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// audio_mel encoder (mel_resnet.hip; mel_resnet.py drives it): log-mel front end, ResNet18 on NHWC activations, projection head
// ------------------------------------------------------------------------------------------------
#define M2F_MEL_NFFT 400
#define M2F_MEL_HOP 160
#define M2F_MEL_BANDS 128
#define M2F_MEL_FRAMES 1001                  // 1 + 160000 / 160: 10 s at 16 kHz
#define M2F_MEL_LOG_EPS 2.220446049250313e-16f
#define M2F_MEL_C0 64                        // stem channels
#define M2F_MEL_STEM_H 501
#define M2F_MEL_STEM_W 64
#define M2F_MEL_POOL_H 251
#define M2F_MEL_POOL_W 32
hipError_t m2f_launch_mel_frontend(const float* wave, const int* lengths, int B, int N, const float* basis, const float* fbT, int levels,
                                   float* peak, float* logmel, float* img, hipStream_t stream);
hipError_t m2f_launch_mel_stem(const float* img, int B, const float* w, const float* bias, float* out32, uint16_t* out16,
                               hipStream_t stream);
hipError_t m2f_launch_mel_conv(const void* x, const void* w, const float* bias, const void* res, void* out, int B, int H, int W, int Cin,
                               int Cout, int ks, int stride, int bf16, int out32, int relu, hipStream_t stream);
hipError_t m2f_launch_mel_head(const void* x, int in16, int B, int HW, int C, const float* w1t, const float* b1, int N1, const float* w2t,
                               const float* b2, int N2, float* out, hipStream_t stream);
