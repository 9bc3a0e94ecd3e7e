// Long-dialogue attention (1 <= L <= 512 utterances per dialogue), forward and backward, for gfx950 (wave64).
//
// The dialogue kernels of attention.hip keep one whole (dialogue, head) in one workgroup and its score tile in one wave's
// registers, which bounds them at L <= 64.  These kernels cut a dialogue into 64-row blocks instead:
//   * forward:  one workgroup per (dialogue, head, 64-query block); K and V stream through LDS in 64-key blocks.  Two passes
//               over the keys: the first finds each query's max and normaliser (online), the second recomputes the scores,
//               writes the normalised P^T (pre-dropout) to the probabilities buffer - same [B*H, Lp, Lp] layout as the short
//               kernels, so the backward needs no recompute - applies dropout and accumulates O = P V.  O needs no rescaling.
//   * backward: one workgroup per (dialogue, head, 64-key block) for dK / dV, looping over query blocks, and one per
//               (dialogue, head, 64-query block) for dQ, looping over key blocks.  Each output row is owned by exactly one
//               workgroup: no atomics, bit-identical from run to run.  D_i = sum_c dO[i][c] O[i][c] is recomputed per query
//               block in both kernels (same code, same order -> same bits).
// Thread shape and arithmetic as attention.hip: 256 threads, wave w owns rows 16w..16w+15 of its block, exact-fp32 MFMA
// v_mfma_f32_16x16x4_f32, and S^T = K Q^T puts the probabilities in the accumulator layout that is the A operand of P V.
// Context band (AttnBatch::band_past / band_future, ops.h): inside a block pair the band is one more term of the key mask; a pair
// of 64-row blocks that the band hides as a whole is SKIPPED by all three kernels through the same test
// (m2f_attn_band_blocks_meet) - the forward leaves that block of the probabilities buffer as it was (a plan's buffer holds the
// previous step's values there) and neither backward kernel reads it.  A query that sees no key gets P = 0 and a zero output row.
// Distance-decay bias (AttnBatch::bias_gain16, ops.h m2f_attn_bias_slope): the forward's BIAS instantiations add -slope_h * |i - j| to the
// scaled score of every visible key, i and j positions in the dialogue (block offset + row on BOTH sides), through dlong_score<> in
// pass 1 and pass 2 alike, so the probabilities are normalised by the sum of exactly the scores they were formed from.  No block pair
// is skipped on its account (a far block's probabilities may underflow; the band's test stays the only skip rule), and the backward
// kernels - dkdv, dq, delta_rows - read the saved probabilities, recompute no score and are not touched by it.
// Speaker heads (AttnBatch::speaker / spk_same / spk_other, ops.h m2f_attn_speaker_class): the forward's SPK instantiations AND one more
// condition into the keys a query sees, beside key_bits() and the band's bits, per 64-key block: the block's speaker ids are read one per
// lane (lane = key) where the pad flags are, a lane gathers the ids of its sixteen score elements' keys with shuffles and tests one byte
// per element against its query's id.  The pattern is not block-shaped, so NO block is skipped on its account (the band's test stays the
// only skip rule) and every element of a visited block is written, a hidden one as 0 - what the attention-maps gather reads.  A query
// that sees no key (an other-speaker head in a monologue) gets P = 0 and a zero output row by the rule above.  The backward kernels
// read the saved probabilities and stay the text they are.
// Both layouts of AttnBatch: packed (cu: dialogue b owns rows cu[b] .. cu[b+1]-1, no pad keys) and padded (key_pad: masked
// keys get -inf before the softmax).  Operands are read as fp32 in both precision modes; results also go to their bf16
// shadows when the plan keeps them (out / dq / dk / dv, and AttnProblem::no_f32 as in attention.hip).
#include "common.h"
#include <algorithm>
#include "ops.h"

// (see attention.hip: no floating-point contraction, so every form of a formula rounds the same way)
#pragma clang fp contract(off)

namespace {

#include "attn_slab.h"

constexpr int BLK = 64;            // rows of a query / key block

// rows [0, n) x cols [0, hd) of src into a zero-padded [BLK x W] LDS slab of row stride ld; register form for W <= 128
__device__ __forceinline__ void stage(float* __restrict__ lds, const float* __restrict__ src, int ldg, int n, int hd, int W, int ld,
                                      int tid) {
    constexpr int NV = 8;
    if (slab_fast_ok<NV>(src, ldg, hd, BLK, W)) {
        SlabGeom<NV> G;
        slab_geom(G, n, hd, BLK, W, ld, tid);
        SlabRegs<NV> R;
        slab_issue(R, G, src, ldg);
        slab_commit(R, G, lds);
    } else {
        load_slab(lds, ld, BLK, W, src, ldg, n, hd, tid);
    }
}

// D_i = sum_c dO[i][c] O[i][c] of the n rows of a block: four lanes per row, dO from its LDS slab, O from global memory
__device__ __forceinline__ void delta_rows(float* __restrict__ delta, const float* __restrict__ Gs, int ld, const float* __restrict__ og,
                                           int ldo, int n, int hd, int tid) {
    const int row = tid >> 2, part = tid & 3;
    const bool ok = row < n;
    const float* o = og + (size_t)(ok ? row : 0) * ldo;
    const float* g = Gs + row * ld;
    float d = 0.f;
    for (int c = part; c < hd; c += 4) d += g[c] * o[c];
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    if (part == 0) delta[row] = ok ? d : 0.f;
}

// C[m][n] = sum_c A[16 t + m][c] B[row n][c] over the head dim: A rows from slab `as` (tile t, row l15), B row `brow`
// -> lane holds C[4 lg + r][l15]
__device__ __forceinline__ f32x4 dot_tile(const float* as, const float* brow, int ksteps) {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    int ks = 0;
    for (; ks + 1 < ksteps; ks += 2) {                     // two accumulators: 40-cycle dependent latency, 32-cycle issue
        acc0 = mfma4(as[4 * ks], brow[4 * ks], acc0);
        acc1 = mfma4(as[4 * ks + 4], brow[4 * ks + 4], acc1);
    }
    if (ks < ksteps) acc0 = mfma4(as[4 * ks], brow[4 * ks], acc0);
    return acc0 + acc1;
}

// dropout keep index of P[i][j] of head bh - the rule of attention.hip, (bh * L + i) * L + j, in unsigned 32-bit arithmetic
// (the plan refuses B * H * L * L >= 2^32, m2f_attn_dlong_index_ok)
__device__ __forceinline__ uint32_t drop_idx(int bh, int L, int i, int j) {
    return ((uint32_t)bh * (uint32_t)L + (uint32_t)i) * (uint32_t)L + (uint32_t)j;
}

// which problem, (dialogue, head) and 64-row block a workgroup owns, and that dialogue's token rows
struct Where {
    int pi, bh, b, h, blk;
    int n;             // rows of the dialogue (packed: its length; padded: the plan's L)
    size_t tok0;       // its first token row
};
__device__ __forceinline__ Where where(const AttnBatch& ab) {
    Where w;
    w.pi = 0;
#pragma unroll
    for (int i = 1; i < M2F_ATTN_MAX_PROBLEMS; ++i)
        if ((int)blockIdx.x >= ab.bb[i]) w.pi = i;
    const int nblk = (ab.L + BLK - 1) / BLK;
    const int idx = (int)blockIdx.x - ab.pr[w.pi].block_begin;
    w.bh = idx / nblk; w.blk = idx - w.bh * nblk;
    w.b = w.bh / ab.pr[w.pi].H; w.h = w.bh - w.b * ab.pr[w.pi].H;
    w.n = ab.L; w.tok0 = (size_t)w.b * ab.L;
    if (ab.cu) {
        const int c0 = ab.cu[w.b], n = ab.cu[w.b + 1] - c0;
        w.n = n < 0 ? 0 : (n > ab.L ? ab.L : n);           // (the probabilities buffer holds L x L per head)
        w.tok0 = (size_t)c0;
    }
    return w;
}

// packed layout: the token rows behind the last dialogue (cu[B] .. T-1) belong to nobody and are written as zeros (see
// attention.hip) - by block 0 of the last dialogue's workgroups, head h its own columns
__device__ __forceinline__ void zero_tail(const AttnBatch& ab, const Where& w, int hd, float* p, int ldp, uint16_t* p16, bool w32,
                                          int lane, int wv) {
    if (!ab.cu || w.b != ab.B - 1 || w.blk != 0 || !p) return;
    for (int r = ab.cu[ab.B] + wv; r < ab.T; r += NWAVE)
        for (int c = lane; c < hd; c += 64) {
            const size_t idx = (size_t)r * ldp + w.h * hd + c;
            if (w32) p[idx] = 0.f;
            if (p16) p16[idx] = 0;
        }
}

// key-valid bits of the key block at kb (nk rows): packed - every row of the dialogue, padded - key_pad == 0
__device__ __forceinline__ unsigned long long key_bits(const AttnBatch& ab, const Where& w, int kb, int nk, int lane) {
    const unsigned char kp = ab.cu ? (unsigned char)0 : ab.key_pad[w.tok0 + kb + (lane < nk ? lane : 0)];
    return __ballot(lane < nk && kp == 0);
}

// the scaled score of query iq and key j (positions in the dialogue); BIAS: plus -slope * |iq - j|, one fma - both passes of the forward
template <bool BIAS>
__device__ __forceinline__ float dlong_score(float acc, float scale, float nslope, int iq, int j) {
    const float x = acc * scale;
    if constexpr (BIAS) return __fmaf_rn(nslope, (float)abs(iq - j), x);
    return x;
}
// SPK: the speaker ids of the keys of this lane's sixteen score elements (keys 16 jt + 4 lg + r of the block at kb), one word per jt
template <bool SPK>
__device__ __forceinline__ void dlong_key_speakers(const AttnBatch& ab, const Where& w, int kb, int nk, int lane, int lg, uint32_t (&spk4)[4]) {
    if constexpr (SPK) {
        const int ks = ab.speaker[w.tok0 + kb + (lane < nk ? lane : 0)];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) spk4[jt] = m2f_spk_pack4(ks, 16 * jt + 4 * lg);
    }
}
// CTM: 16-column tiles of the head dim held in registers (8: hd <= 128, 16: hd <= 256); BAND: the launch has a context band (its
// own instantiations of the three kernels, so that a launch without one runs the code it always ran); BIAS (forward only): it has a
// distance-decay bias - instantiations of their own again; SPK (forward only): it has speaker heads - likewise
template <int CTM, bool BAND, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(NTHR) void m2f_attn_dlong_fwd_kernel(const AttnBatch ab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const Where w = where(ab);
    const AttnProblem& P = ab.pr[w.pi];
    const int LM = ab.L, Lp = 16 * ((LM + 15) >> 4), hd = P.hd, W = (hd + 15) & ~15, ld = W + 2, CT = W >> 4;
    uint16_t* out16 = m2f_shadow_of(ab.sh, P.out);
    const bool w32 = !(P.no_f32 && out16);                  // (no fp32 reader: the bf16 shadow is the result)
    zero_tail(ab, w, hd, P.out, P.ldo, out16, w32, lane, wv);
    const int q0 = w.blk * BLK;
    if (q0 >= w.n) return;                                  // (packed: a dialogue shorter than the plan's L)
    float* Qs = sm;
    float* KV = Qs + BLK * ld;                              // K, then V, of the current key block
    stage(Qs, P.q + (w.tok0 + q0) * P.ldq + w.h * hd, P.ldq, min(BLK, w.n - q0), hd, W, ld, tid);

    const float scale = 1.0f / sqrtf((float)hd);
    const int ksteps = (hd + 3) >> 2;
    const int i = 16 * wv + l15, iq = q0 + i;               // this lane's query row (block-local / in the dialogue)
    const float* qrow = Qs + i * ld + lg;
    const float* kb_rows = KV + l15 * ld + lg;
    float nslope = 0.f;                                     // BIAS: minus the head's slope
    if constexpr (BIAS) nslope = -m2f_attn_bias_slope(w.h, P.H, m2f_attn_bias_gain(ab.bias_gain16));
    int spk_cls = M2F_SPK_NONE, mine = 0;                   // SPK: the head's class (uniform per workgroup), this lane's query's speaker
    uint32_t spk4[4] = {0u, 0u, 0u, 0u};
    if constexpr (SPK) {
        spk_cls = m2f_attn_speaker_class(w.h, ab.spk_same, ab.spk_other);
        mine = ab.speaker[w.tok0 + (iq < w.n ? iq : w.n - 1)];          // (q0 < w.n: w.n >= 1)
    }

    // pass 1: row max and normaliser
    float m_run = -INFINITY, l_run = 0.f;
    for (int kb = 0; kb < w.n; kb += BLK) {
        if (BAND && !m2f_attn_band_blocks_meet(ab, q0, kb)) continue;     // (block-uniform; pass 2 and both backward kernels skip the same pairs)
        const int nk = min(BLK, w.n - kb);
        __syncthreads();                                    // previous K / V block consumed (and Q committed)
        stage(KV, P.k + (w.tok0 + kb) * P.ldk + w.h * hd, P.ldk, nk, hd, W, ld, tid);
        unsigned long long kvalid = key_bits(ab, w, kb, nk, lane);
        if constexpr (BAND) kvalid &= m2f_attn_band_bits(ab, iq, kb);     // (from here on per lane: the keys its query sees)
        dlong_key_speakers<SPK>(ab, w, kb, nk, lane, lg, spk4);
        __syncthreads();
        float s[4][4];
        float m_blk = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 acc = dot_tile(kb_rows + 16 * jt * ld, qrow, ksteps);    // S[i][j = 16jt + 4lg + r]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * lg + r;
                bool on = (kvalid >> j) & 1ull;
                if constexpr (SPK) on = on && m2f_spk_sees(spk_cls, spk4[jt], r, mine);
                s[jt][r] = on ? dlong_score<BIAS>(acc[r], scale, nslope, iq, kb + j) : -INFINITY;
                m_blk = fmaxf(m_blk, s[jt][r]);
            }
        }
        m_blk = fmaxf(m_blk, __shfl_xor(m_blk, 16, 64));
        m_blk = fmaxf(m_blk, __shfl_xor(m_blk, 32, 64));
        const float m_new = fmaxf(m_run, m_blk);
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += (m_new == -INFINITY) ? 0.f : __expf(s[jt][r] - m_new);
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * ((m_new == -INFINITY) ? 1.f : __expf(m_run - m_new)) + sum;
        m_run = m_new;
    }

    // pass 2: P = exp(S - m) / l -> P^T (pre-dropout) to probs, dropout, O += P V
    const float inv = (iq < w.n && l_run > 0.f) ? 1.0f / l_run : 0.f;      // rows past the dialogue, rows that see no key: P = 0
    const uint32_t site = P.drop_site;
    uint32_t key = 0;
    if (site) key = m2f_site_key(ab.rng, site);
    float* probs = P.probs + (size_t)w.bh * Lp * Lp;
    f32x4 o[CTM];
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < w.n; kb += BLK) {
        if (BAND && !m2f_attn_band_blocks_meet(ab, q0, kb)) continue;     // (its block of probs keeps what it held: the backward skips it too)
        const int nk = min(BLK, w.n - kb);
        __syncthreads();
        stage(KV, P.k + (w.tok0 + kb) * P.ldk + w.h * hd, P.ldk, nk, hd, W, ld, tid);
        unsigned long long kvalid = key_bits(ab, w, kb, nk, lane);
        if constexpr (BAND) kvalid &= m2f_attn_band_bits(ab, iq, kb);
        dlong_key_speakers<SPK>(ab, w, kb, nk, lane, lg, spk4);
        __syncthreads();
        float p[4][4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 acc = dot_tile(kb_rows + 16 * jt * ld, qrow, ksteps);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jl = 16 * jt + 4 * lg + r, j = kb + jl;
                bool on = (kvalid >> jl) & 1ull;
                if constexpr (SPK) on = on && m2f_spk_sees(spk_cls, spk4[jt], r, mine);
                const float x = on ? dlong_score<BIAS>(acc[r], scale, nslope, iq, j) : -INFINITY;
                float pv = (m_run == -INFINITY) ? 0.f : __expf(x - m_run) * inv;   // (no visible key: exp(-inf + inf) would be NaN)
                if (iq < Lp && j < Lp) probs[(size_t)j * Lp + iq] = pv;           // lanes: consecutive iq
                if (site) pv = m2f_keep(key, drop_idx(w.bh, LM, iq, j), ab.drop_thresh) ? pv * ab.drop_scale : 0.f;
                p[jt][r] = pv;
            }
        }
        __syncthreads();                                    // K consumed
        stage(KV, P.v + (w.tok0 + kb) * P.ldv + w.h * hd, P.ldv, nk, hd, W, ld, tid);
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < CTM; ++ct) {                  // static indices keep o[] in registers
            if (ct >= CT) continue;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const float* vp = KV + (16 * jt + 4 * lg) * ld + 16 * ct + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[ct] = mfma4(p[jt][r], vp[r * ld], o[ct]);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) {
        if (ct >= CT) continue;
        const int c = 16 * ct + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int io = q0 + 16 * wv + 4 * lg + r;
            if (io < w.n && c < hd) {
                const size_t idx = (w.tok0 + io) * P.ldo + w.h * hd + c;
                if (w32) P.out[idx] = o[ct][r];
                if (out16) out16[idx] = m2f_bf16_bits(o[ct][r]);
            }
        }
    }
}

// dK = scale dS^T Q, dV = P~^T dO for the 64 keys of one block; lane = key (l15), registers = query rows
template <int CTM, bool BAND>
__global__ __launch_bounds__(NTHR) void m2f_attn_dlong_dkdv_kernel(const AttnBatch ab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const Where w = where(ab);
    const AttnProblem& P = ab.pr[w.pi];
    const int LM = ab.L, Lp = 16 * ((LM + 15) >> 4), hd = P.hd, W = (hd + 15) & ~15, ld = W + 2, CT = W >> 4;
    uint16_t* dq16 = m2f_shadow_of(ab.sh, P.dq);
    uint16_t* dk16 = m2f_shadow_of(ab.sh, P.dk);
    uint16_t* dv16 = m2f_shadow_of(ab.sh, P.dv);
    const bool w32 = !(P.no_f32 && dq16 && dk16 && dv16);
    zero_tail(ab, w, hd, P.dk, P.lddk, dk16, w32, lane, wv);
    zero_tail(ab, w, hd, P.dv, P.lddv, dv16, w32, lane, wv);
    const int j0 = w.blk * BLK;
    if (j0 >= w.n) return;
    float* Vs = sm;                                         // V of this key block (resident)
    float* X = Vs + BLK * ld;                               // dO, then Q, of the current query block
    float* delta = X + BLK * ld;                            // [BLK]
    stage(Vs, P.v + (w.tok0 + j0) * P.ldv + w.h * hd, P.ldv, min(BLK, w.n - j0), hd, W, ld, tid);

    const float scale = 1.0f / sqrtf((float)hd);
    const int ksteps = (hd + 3) >> 2;
    const int j = j0 + 16 * wv + l15;                       // this lane's key
    const float* vrow = Vs + (16 * wv + l15) * ld + lg;
    const uint32_t site = P.drop_site;
    uint32_t key = 0;
    if (site) key = m2f_site_key(ab.rng, site);
    const float* pt = P.probs + (size_t)w.bh * Lp * Lp + (size_t)(j < w.n ? j : 0) * Lp;     // row j of P^T
    f32x4 dk[CTM], dv[CTM];
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) { dk[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[ct] = dk[ct]; }
    for (int qb = 0; qb < w.n; qb += BLK) {
        if (BAND && !m2f_attn_band_blocks_meet(ab, qb, j0)) continue;     // (the forward wrote no probabilities for this pair: all zero under the band)
        const int nq = min(BLK, w.n - qb);
        __syncthreads();                                    // previous Q slab consumed
        stage(X, P.dout + (w.tok0 + qb) * P.lddo + w.h * hd, P.lddo, nq, hd, W, ld, tid);
        __syncthreads();
        delta_rows(delta, X, ld, P.out + (w.tok0 + qb) * P.ldo + w.h * hd, P.ldo, nq, hd, tid);
        __syncthreads();
        float ds[4][4], pd[4][4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const f32x4 acc = dot_tile(X + (16 * it + l15) * ld + lg, vrow, ksteps);       // dP[i = 16it + 4lg + r][j]
            const int ib = qb + 16 * it + 4 * lg;
            const bool live = j < w.n && qb + 16 * it < w.n;
            const f32x4 p4 = live ? *reinterpret_cast<const f32x4*>(pt + ib) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ib + r;
                const float p = (live && i < w.n) ? p4[r] : 0.f;
                float dp = acc[r], pdv = p;
                if (site) {
                    const bool kp = m2f_keep(key, drop_idx(w.bh, LM, i, j), ab.drop_thresh);
                    dp = kp ? dp * ab.drop_scale : 0.f;
                    pdv = kp ? p * ab.drop_scale : 0.f;
                }
                ds[it][r] = p * (dp - delta[16 * it + 4 * lg + r]) * scale;
                pd[it][r] = pdv;
            }
        }
#pragma unroll
        for (int ct = 0; ct < CTM; ++ct) {
            if (ct >= CT) continue;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const float* gp = X + (16 * it + 4 * lg) * ld + 16 * ct + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) dv[ct] = mfma4(pd[it][r], gp[r * ld], dv[ct]);
            }
        }
        __syncthreads();                                    // dO consumed
        stage(X, P.q + (w.tok0 + qb) * P.ldq + w.h * hd, P.ldq, nq, hd, W, ld, tid);
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < CTM; ++ct) {
            if (ct >= CT) continue;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const float* qp = X + (16 * it + 4 * lg) * ld + 16 * ct + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) dk[ct] = mfma4(ds[it][r], qp[r * ld], dk[ct]);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) {
        if (ct >= CT) continue;
        const int c = 16 * ct + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jo = j0 + 16 * wv + 4 * lg + r;
            if (jo < w.n && c < hd) {
                const size_t ik = (w.tok0 + jo) * P.lddk + w.h * hd + c, iv = (w.tok0 + jo) * P.lddv + w.h * hd + c;
                if (w32) { P.dk[ik] = dk[ct][r]; P.dv[iv] = dv[ct][r]; }
                if (dk16) dk16[ik] = m2f_bf16_bits(dk[ct][r]);
                if (dv16) dv16[iv] = m2f_bf16_bits(dv[ct][r]);
            }
        }
    }
}

// dQ = scale dS K for the 64 queries of one block; lane = query (l15), registers = keys
template <int CTM, bool BAND>
__global__ __launch_bounds__(NTHR) void m2f_attn_dlong_dq_kernel(const AttnBatch ab) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const Where w = where(ab);
    const AttnProblem& P = ab.pr[w.pi];
    const int LM = ab.L, Lp = 16 * ((LM + 15) >> 4), hd = P.hd, W = (hd + 15) & ~15, ld = W + 2, CT = W >> 4;
    uint16_t* dq16 = m2f_shadow_of(ab.sh, P.dq);
    uint16_t* dk16 = m2f_shadow_of(ab.sh, P.dk);
    uint16_t* dv16 = m2f_shadow_of(ab.sh, P.dv);
    const bool w32 = !(P.no_f32 && dq16 && dk16 && dv16);
    zero_tail(ab, w, hd, P.dq, P.lddq, dq16, w32, lane, wv);
    const int q0 = w.blk * BLK;
    if (q0 >= w.n) return;
    float* Gs = sm;                                         // dO of this query block (resident)
    float* KV = Gs + BLK * ld;                              // V, then K, of the current key block
    float* delta = KV + BLK * ld;                           // [BLK]
    const int nq = min(BLK, w.n - q0);
    stage(Gs, P.dout + (w.tok0 + q0) * P.lddo + w.h * hd, P.lddo, nq, hd, W, ld, tid);
    __syncthreads();
    delta_rows(delta, Gs, ld, P.out + (w.tok0 + q0) * P.ldo + w.h * hd, P.ldo, nq, hd, tid);
    __syncthreads();

    const float scale = 1.0f / sqrtf((float)hd);
    const int ksteps = (hd + 3) >> 2;
    const int i = 16 * wv + l15, iq = q0 + i;               // this lane's query (block-local / in the dialogue)
    const float dl = delta[i];
    const float* grow = Gs + i * ld + lg;
    const uint32_t site = P.drop_site;
    uint32_t key = 0;
    if (site) key = m2f_site_key(ab.rng, site);
    const float* probs = P.probs + (size_t)w.bh * Lp * Lp;
    f32x4 dq[CTM];
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) dq[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < w.n; kb += BLK) {
        if (BAND && !m2f_attn_band_blocks_meet(ab, q0, kb)) continue;     // (as the forward and dK / dV)
        const int nk = min(BLK, w.n - kb);
        __syncthreads();                                    // previous K slab consumed
        stage(KV, P.v + (w.tok0 + kb) * P.ldv + w.h * hd, P.ldv, nk, hd, W, ld, tid);
        __syncthreads();
        float ds[4][4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 acc = dot_tile(KV + (16 * jt + l15) * ld + lg, grow, ksteps);      // dP[i][j = kb + 16jt + 4lg + r]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jj = kb + 16 * jt + 4 * lg + r;
                const float p = (iq < w.n && jj < w.n) ? probs[(size_t)jj * Lp + iq] : 0.f;
                float dp = acc[r];
                if (site) dp = m2f_keep(key, drop_idx(w.bh, LM, iq, jj), ab.drop_thresh) ? dp * ab.drop_scale : 0.f;
                ds[jt][r] = p * (dp - dl) * scale;
            }
        }
        __syncthreads();                                    // V consumed
        stage(KV, P.k + (w.tok0 + kb) * P.ldk + w.h * hd, P.ldk, nk, hd, W, ld, tid);
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < CTM; ++ct) {
            if (ct >= CT) continue;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const float* kp = KV + (16 * jt + 4 * lg) * ld + 16 * ct + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) dq[ct] = mfma4(ds[jt][r], kp[r * ld], dq[ct]);
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CTM; ++ct) {
        if (ct >= CT) continue;
        const int c = 16 * ct + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int io = q0 + 16 * wv + 4 * lg + r;
            if (io < w.n && c < hd) {
                const size_t idx = (w.tok0 + io) * P.lddq + w.h * hd + c;
                if (w32) P.dq[idx] = dq[ct][r];
                if (dq16) dq16[idx] = m2f_bf16_bits(dq[ct][r]);
            }
        }
    }
}

// grid = sum over problems of B * H * ceil(L / 64) workgroups; returns the widest padded head dim, or -1 for a bad batch
int prepare(AttnBatch& ab, int& blocks) {
    if (ab.count <= 0 || ab.count > M2F_ATTN_MAX_PROBLEMS || ab.B < 1 || ab.L < 1 || ab.L > M2F_ATTN_DLONG_MAX_L) return -1;
    if (!ab.cu && !ab.key_pad) return -1;
    const int nblk = (ab.L + BLK - 1) / BLK;
    int maxW = 0;
    blocks = 0;
    for (int i = 0; i < M2F_ATTN_MAX_PROBLEMS; ++i) ab.bb[i] = 0x7fffffff;
    for (int i = 0; i < ab.count; ++i) {
        AttnProblem& p = ab.pr[i];
        if (p.hd < 1 || p.hd > 256 || p.H < 1) return -1;
        if (p.drop_site && !ab.rng) return -1;
        if (!m2f_attn_dlong_index_ok(ab.B, p.H, ab.L)) return -1;
        p.block_begin = blocks;
        ab.bb[i] = blocks;
        blocks += ab.B * p.H * nblk;
        maxW = std::max(maxW, (p.hd + 15) & ~15);
    }
    return maxW;
}

template <typename K>
hipError_t go(K kern, int blocks, size_t lds, hipStream_t stream, const AttnBatch& ab) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NTHR), lds, stream, ab);
    return hipGetLastError();
}

bool has_band(const AttnBatch& ab) { return (ab.band_past | ab.band_future) != 0; }

}  // namespace

bool m2f_attn_dlong_index_ok(int B, int H, int L) {
    return (uint64_t)B * (uint64_t)H * (uint64_t)L * (uint64_t)L < (1ull << 32);
}

hipError_t m2f_launch_attn_dlong_fwd(AttnBatch& ab, hipStream_t stream) {
    int blocks = 0;
    const int maxW = prepare(ab, blocks);
    if (maxW < 0) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * BLK * (maxW + 2) * sizeof(float);
    const bool spk = (ab.spk_same | ab.spk_other) != 0;
    if (spk && !m2f_attn_speakers_ok(ab)) return hipErrorInvalidValue;
    return m2f_pick_bools([&](auto WIDE, auto BAND, auto BIAS, auto SPK) {         // one instantiation per combination of the four flags
        return go(m2f_attn_dlong_fwd_kernel<WIDE.value ? 16 : 8, BAND.value, BIAS.value, SPK.value>, blocks, lds, stream, ab);
    }, maxW > 128, has_band(ab), ab.bias_gain16 != 0, spk);
}

hipError_t m2f_launch_attn_dlong_bwd(AttnBatch& ab, hipStream_t stream) {
    int blocks = 0;
    const int maxW = prepare(ab, blocks);
    if (maxW < 0) return hipErrorInvalidValue;
    const size_t lds = ((size_t)2 * BLK * (maxW + 2) + BLK) * sizeof(float);
    return m2f_pick_bools([&](auto WIDE, auto BAND) {
        constexpr int CTM = WIDE.value ? 16 : 8;
        const hipError_t e = go(m2f_attn_dlong_dkdv_kernel<CTM, BAND.value>, blocks, lds, stream, ab);
        return e != hipSuccess ? e : go(m2f_attn_dlong_dq_kernel<CTM, BAND.value>, blocks, lds, stream, ab);
    }, maxW > 128, has_band(ab));
}
