// Streaming ("prefill") dialogue attention on gfx950: UP TO T NEW UTTERANCES per live dialogue in one launch, against that dialogue's
// cached keys / values and against each other under the stream's band.
//
// The problem is (stream slot s, head h): the slot's n_new[s] (0 .. T, T <= 64) new query rows - rows s*T + t of q / k / v - against the
// n_old = len[s] utterances the slot has cached plus the chunk's own rows.  The defining rule is attention_stream.hip's, row by row: a
// chunk of n rows gives what n single-row launches give.  Query t is utterance u = n_old + t; it sees the chunk's rows <= t and
//   * plain cache: every cached utterance (n_old + n_new <= C required: a slot that would pass C is treated as not live);
//   * ring of C rows (a window of C - 1): the utterances u - (C - 1) .. u only; utterance j lives in cache row j % C.
// Cache layout, padding and element types are attention_stream.hip's (cache[S][H][C][hdp], fp32 or bf16): a step and a chunk call
// interleave on the same caches.
// The caches may also be page pools (attention_stream.hip has both layouts): logical cache row j of the slot is then row j % R of page
// table[s][j / R].  A 64-row block of cached rows starts at a multiple of 64 logical rows, so it is 64 / R whole pages; the staging
// takes each row from its page, the ids coming from LDS, where the workgroup put the slot's table entries once (attn_stream_rows.h:
// only the entries of pages that hold a live row or take a new one, e < ceil(min(len + n_new, C) / R)).  Dense and paged are ONE
// kernel body (attn_stream_chunk_body<BF16, PAGED>); behind PAGED stand only that fetch, the base pointer of a head's rows and the
// offset of a row, so the output and the rows stored are the same bits in both.
//
// One workgroup of 4 waves per (s, h), the shape and arithmetic of attention_dlong.hip's forward with one query block: wave w owns the
// queries 16w .. 16w + 15, exact-fp32 MFMA v_mfma_f32_16x16x4_f32, S^T = K Q^T so that the probabilities come out in the layout that is
// the A operand of P V.  Q and the chunk's own K / V stay in LDS for the whole launch (bf16 mode: rounded there once - the values the
// cache will hold); the cached rows stream through a fourth slab in 64-row blocks (bf16 caches are widened on the way in), in cache-row
// order.  Two passes over the keys - row max and normaliser, then P and O += P V - in fp32, scale applied to the fp32 product.
// The chunk's own keys are NEVER read through the cache.  On a ring the new rows overwrite rows that earlier queries of the same chunk
// still need, so every store of a new row comes after the workgroup's last cache read, behind a barrier; of n_new > C new rows only
// the last C are stored (the others would be overwritten inside the launch).  The row a ring is about to recycle for the chunk's
// first utterance is dead to every query and is not read at all.  No atomics, one summation order: the same bits on every run.
// len[] is NOT advanced here: every site of a prefill call reads the same counts, m2f_launch_stream_advance_n closes the call.
// BIAS (a third flag of the body, its own instantiations): the launch has a distance-decay bias (ops.h, m2f_attn_bias_slope;
// AttnStreamBatch::bias_gain).  Query t is utterance n_old + t, a cached row at logical index d utterance n_old - nlive + d, an own row
// t' utterance n_old + t'; both passes add -slope * distance through biased<>, so they form the identical score.
// SPK (a fourth flag, its own instantiations): the launch has speaker heads (ops.h, m2f_attn_speaker_class).  The one rule of the step
// kernel, for cached rows and for the chunk's own rows alike: query t carries spk_new[s][t], a cached row its byte of spk_cache[s] (logical
// row = cache row, read 64 at a time with the block they belong to, lane = row), an own row t' spk_new[s][t']; a lane gathers the ids of
// its sixteen score elements' keys with shuffles (ops.h, m2f_spk_pack4) and both passes AND the same test into the visibility.  A query
// whose head sees no row - an other-speaker head before another speaker has spoken - gets a zero output row (m_run stays -inf, as for a
// band).  spk_cache is only read here; m2f_launch_stream_advance_speakers_n stores the chunk's ids behind the call's last attention launch.
#include "common.h"
#include "ops.h"
#include "attn_stream_rows.h"

// (see attention.hip: no floating-point contraction, so every form of a formula rounds the same way)
#pragma clang fp contract(off)

namespace {

#include "attn_slab.h"

constexpr int BLK = 64;            // rows of the query block / of a key block
constexpr int NV = 8;              // float4 per thread of a [BLK x 128] slab

__device__ __forceinline__ float round_bf16(float x) { return m2f_bf16_to_f32(m2f_bf16_bits(x)); }

// rows [0, n) x cols [0, hd) of a strided fp32 operand into a zero-padded [BLK x W] slab (bf16 mode: rounded once); rows >= n are
// never read
template <bool BF16>
__device__ __forceinline__ void stage_new(float* __restrict__ lds, const float* __restrict__ src, int ldg, int n, int hd, int W, int ld,
                                          int tid) {
    if (slab_fast_ok<NV>(src, ldg, hd, BLK, W)) {
        SlabGeom<NV> G;
        slab_geom(G, n, hd, BLK, W, ld, tid);
        SlabRegs<NV> R;
        slab_issue(R, G, src, ldg);
        if (BF16) {
#pragma unroll
            for (int u = 0; u < NV; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) R.x[u][i] = round_bf16(R.x[u][i]);
        }
        slab_commit(R, G, lds);
        return;
    }
    const int total = BLK * W;
#pragma unroll 1
    for (int base = 0; base < total; base += NTHR * 4) {
        float x[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = base + tid + NTHR * u;
            const int r = e / W, c = e - r * W;
            const bool ok = e < total && r < n && c < hd;
            off[u] = e < total ? r * ld + c : -1;
            x[u] = src[ok ? (size_t)r * ldg + c : (size_t)0];
            x[u] = ok ? (BF16 ? round_bf16(x[u]) : x[u]) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) lds[off[u]] = x[u];
    }
}

// cache rows [r0, r0 + n) of one (slot, head) into a zero-padded [BLK x W] slab; the row `dead` (absolute; -1: none) is not read.
// Rows are hdp elements wide and 16-byte aligned, their pad columns hold zeros.  cache: the head's row 0 (dense) or its row 0 of page
// 0 (paged: spg, lgR, page_stride say where a row is).  Loads are unconditional: a slot outside the block reads the block's first row.
template <bool BF16, bool PAGED>
__device__ __forceinline__ void stage_cache(float* __restrict__ lds, const void* __restrict__ cache, const int* __restrict__ spg, int lgR,
                                            size_t page_stride, int r0, int n, int dead, int hdp, int W, int ld, int tid) {
    SlabGeom<NV> G;
    slab_geom(G, n, hdp, BLK, W, ld, tid);
    SlabRegs<NV> R;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int r = G.goff_rc[u] >> 16, c = G.goff_rc[u] & 0xFFFF;
        G.ok[u] = G.ok[u] && (r0 + r) != dead;
        size_t o;
        if (PAGED) o = m2f_stream_row_off(spg, lgR, page_stride, G.ok[u] ? r0 + r : r0, hdp, G.ok[u] ? c : 0);
        else o = (size_t)r0 * hdp + (size_t)(G.ok[u] ? (uint32_t)(r * hdp + c) : 0u);
        if (BF16) {
            const uint2 w = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(cache) + o);
            R.w0[u] = w.x; R.w1[u] = w.y;
        } else {
            R.x[u] = *reinterpret_cast<const f32x4*>(static_cast<const float*>(cache) + o);
        }
    }
    slab_commit(R, G, lds, BF16);
}

// C[m][n] = sum_c A[row m][c] B[row n][c] over the head dim (attention_dlong.hip) -> lane holds C[4 lg + r][l15]
__device__ __forceinline__ f32x4 dot_tile(const float* as, const float* brow, int ksteps) {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    int ks = 0;
    for (; ks + 1 < ksteps; ks += 2) {
        acc0 = mfma4(as[4 * ks], brow[4 * ks], acc0);
        acc1 = mfma4(as[4 * ks + 4], brow[4 * ks + 4], acc1);
    }
    if (ks < ksteps) acc0 = mfma4(as[4 * ks], brow[4 * ks], acc0);
    return acc0 + acc1;
}

// What query i of the chunk sees.  Cached rows are walked in cache-row order; on a ring row r holds the utterance that is d(r) places
// behind the oldest live one, d(r) = (r - p0) mod C, p0 = the oldest live utterance's row.
struct Vis {
    int ring, C, nlive, p0, n_new;
    // BIAS: utterances between query i and cache row r (r live and visible to i); chunk row t <= i is i - t behind
    __device__ __forceinline__ int cached_dist(int i, int r) const { return i + nlive - (ring ? r - p0 + (r < p0 ? C : 0) : r); }
    // cache row r (r < nlive: it holds a live utterance) - its utterance j = n_old - nlive + d, visible iff j >= n_old + i - (C - 1)
    __device__ __forceinline__ bool cached(int i, int r) const {
        if (r >= nlive) return false;
        if (!ring) return true;
        const int d = r - p0 + (r < p0 ? C : 0);
        return d >= i + nlive - C + 1;
    }
    // chunk row t
    __device__ __forceinline__ bool own(int i, int t) const { return t < n_new && t <= i && (!ring || t >= i - (C - 1)); }
};

// the score of a visible key `dist` utterances behind its query: x = the scaled fp32 product; BIAS: plus -slope * dist, one fma - the one
// statement both passes go through
template <bool BIAS>
__device__ __forceinline__ float biased(float x, float nslope, int dist) {
    if constexpr (BIAS) return __fmaf_rn(nslope, (float)dist, x);
    return x;
}

template <bool BF16, bool PAGED, bool BIAS, bool SPK = false>
__device__ __forceinline__ void attn_stream_chunk_body(const AttnStreamBatch& ab, const AttnStreamPaging& pg, const int T,
                                                       const int* __restrict__ new_count) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ int spg[32];                                 // paged: the slot's page ids, entry e = logical rows e*R .. e*R + R - 1
    typedef Row<BF16> R;
    typedef typename R::elem_t elem_t;
    constexpr int EPL = R::EPL;                             // elements of a 16-byte access
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < M2F_ATTN_MAX_PROBLEMS; ++i)
        if ((int)blockIdx.x >= ab.bb[i]) pi = i;
    const AttnStreamProblem& P = ab.pr[pi];
    const int local = (int)blockIdx.x - ab.bb[pi];
    const int s = local / P.H, h = local - s * P.H;
    const int hd = P.hd, C = ab.C, W = (hd + 15) & ~15, ld = W + 2, CT = W >> 4;
    const int hdp = m2f_stream_hdp(hd, BF16);
    const size_t row0 = (size_t)s * T;                      // the slot's first row of q / k / v / out
    uint16_t* out16 = m2f_shadow_of(ab.sh, P.out);

    const int n_old = ab.len[s];
    const int n_new = min(new_count[s], T);
    const bool live = n_new > 0 && n_old >= 0 && (ab.ring || (n_old <= C && n_new <= C - n_old));
    {   // rows that take nothing: zero output rows
        const int first = live ? n_new : 0;
        for (int e = tid; e < (T - first) * hd; e += NTHR) {
            const int t = e / hd, c = e - t * hd;
            const size_t idx = (row0 + first + t) * P.ldo + (size_t)h * hd + c;
            P.out[idx] = 0.f;
            if (out16) out16[idx] = 0;
        }
    }
    if (!live) return;                                      // cache and len untouched

    const int lgR = PAGED ? pg.lgR : 0;
    if (PAGED) m2f_stream_page_ids(spg, pg, s, n_old < C - n_new ? n_old + n_new : C, tid);      // rows: min(n_old + n_new, C) without overflow
    float* Qs = sm;
    float* Ks = Qs + BLK * ld;                              // the chunk's own K / V: resident (what the cache will hold)
    float* Vs = Ks + BLK * ld;
    float* KV = Vs + BLK * ld;                              // cached K, then V, of the current block
    stage_new<BF16>(Qs, P.q + row0 * P.ldq + (size_t)h * hd, P.ldq, n_new, hd, W, ld, tid);
    stage_new<BF16>(Ks, P.k + row0 * P.ldk + (size_t)h * hd, P.ldk, n_new, hd, W, ld, tid);
    stage_new<BF16>(Vs, P.v + row0 * P.ldv + (size_t)h * hd, P.ldv, n_new, hd, W, ld, tid);

    // row 0 of the head: of the slot's cache (dense) or of page 0 (paged), and from there to logical row j
    const size_t page_stride = (size_t)P.H * (size_t)(hdp << lgR);           // paged: elements of one page, all heads
    const size_t head0 = PAGED ? (size_t)h * (size_t)(hdp << lgR) : ((size_t)s * P.H + h) * (size_t)C * hdp;
    elem_t* kc = static_cast<elem_t*>(P.kcache) + head0;
    elem_t* vc = static_cast<elem_t*>(P.vcache) + head0;
    const int nlive = min(n_old, C);                        // cache rows that hold a live utterance (ring: the last C)
    Vis vis;
    vis.ring = ab.ring; vis.C = C; vis.nlive = nlive; vis.p0 = ab.ring ? (n_old - nlive) % C : 0; vis.n_new = n_new;
    const int dead = (ab.ring && nlive == C) ? vis.p0 : -1; // the row the chunk's first utterance recycles: outside every query's window

    const float scale = 1.0f / sqrtf((float)hd);
    float nslope = 0.f;                                     // BIAS: minus the head's slope
    if constexpr (BIAS) nslope = -m2f_attn_bias_slope(h, P.H, ab.bias_gain);
    const int ksteps = (hd + 3) >> 2;
    const int i = 16 * wv + l15;                            // this lane's query
    const bool wave_on = 16 * wv < n_new;                   // (wave-uniform: a wave without a query only stages)
    const float* qrow = Qs + i * ld + lg;
    const float* kv_rows = KV + l15 * ld + lg;
    const float* own_rows = Ks + l15 * ld + lg;
    // SPK: the head's class (uniform per workgroup), this lane's query's speaker, the ids of the own keys of its score elements - and,
    // per cached block, of the cached ones (cached_ids / cached_speakers below)
    int spk_cls = M2F_SPK_NONE, mine = 0;
    uint32_t own4[4] = {0u, 0u, 0u, 0u}, spk4[4] = {0u, 0u, 0u, 0u};
    if constexpr (SPK) {
        spk_cls = m2f_attn_speaker_class(h, ab.spk_same, ab.spk_other);
        const uint8_t* nrow = ab.spk_new + row0;            // (n_new >= 1 here)
        mine = nrow[i < n_new ? i : n_new - 1];
        const int ko = nrow[lane < n_new ? lane : 0];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) own4[jt] = m2f_spk_pack4(ko, 16 * jt + 4 * lg);
    }
    // the block's ids are ISSUED with the block's K rows, in front of the barrier that commits them (lane = row; every wave, so that
    // the load is in flight beside stage_cache's and costs no round trip of its own), and gathered behind it
    auto cached_ids = [&](int kb, int nk) -> int {
        if constexpr (SPK) return ab.spk_cache[(size_t)s * C + kb + (lane < nk ? lane : 0)];
        return 0;
    };
    auto cached_speakers = [&](int kc_id) {                 // (every lane of the wave: the shuffles need them all)
        if constexpr (SPK) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) spk4[jt] = m2f_spk_pack4(kc_id, 16 * jt + 4 * lg);
        }
    };
    __syncthreads();                                        // Q, the chunk's K / V and the page ids committed

    // ---- pass 1: row max and normaliser -----------------------------------------------------------------------------------------
    float m_run = -INFINITY, l_run = 0.f;
    auto stats = [&](const float (&x)[4][4]) {
        float m_blk = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) m_blk = fmaxf(m_blk, x[jt][r]);
        m_blk = fmaxf(m_blk, __shfl_xor(m_blk, 16, 64));
        m_blk = fmaxf(m_blk, __shfl_xor(m_blk, 32, 64));
        const float m_new = fmaxf(m_run, m_blk);
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += (m_new == -INFINITY) ? 0.f : __expf(x[jt][r] - m_new);
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * ((m_new == -INFINITY) ? 1.f : __expf(m_run - m_new)) + sum;
        m_run = m_new;
    };
    for (int kb = 0; kb < nlive; kb += BLK) {
        __syncthreads();                                    // previous block consumed
        stage_cache<BF16, PAGED>(KV, kc, spg, lgR, page_stride, kb, min(BLK, nlive - kb), dead, hdp, W, ld, tid);
        const int ids = cached_ids(kb, min(BLK, nlive - kb));
        __syncthreads();
        if (wave_on) {
            float x[4][4];
            cached_speakers(ids);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const f32x4 acc = dot_tile(kv_rows + 16 * jt * ld, qrow, ksteps);      // S[i][j = 16jt + 4lg + r]
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    x[jt][r] = (vis.cached(i, kb + 16 * jt + 4 * lg + r) && (!SPK || m2f_spk_sees(spk_cls, spk4[jt], r, mine)))
                                   ? biased<BIAS>(acc[r] * scale, nslope, BIAS ? vis.cached_dist(i, kb + 16 * jt + 4 * lg + r) : 0) : -INFINITY;
            }
            stats(x);
        }
    }
    if (wave_on) {                                          // the chunk's own keys, from LDS
        float x[4][4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 acc = dot_tile(own_rows + 16 * jt * ld, qrow, ksteps);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                x[jt][r] = (vis.own(i, 16 * jt + 4 * lg + r) && (!SPK || m2f_spk_sees(spk_cls, own4[jt], r, mine))) ? biased<BIAS>(acc[r] * scale, nslope, i - (16 * jt + 4 * lg + r)) : -INFINITY;
        }
        stats(x);
    }

    // ---- pass 2: P = exp(S - m) / l, O += P V ------------------------------------------------------------------------------------------
    const float inv = (i < n_new && l_run > 0.f) ? 1.0f / l_run : 0.f;     // (a query always sees itself: l_run >= 1 for i < n_new - but for SPK, where an other-speaker head may see no row)
    f32x4 o[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto pv = [&](const float (&p)[4][4], const float* vslab) {
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {                    // static indices keep o[] in registers
            if (ct >= CT) continue;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const float* vp = vslab + (16 * jt + 4 * lg) * ld + 16 * ct + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[ct] = mfma4(p[jt][r], vp[r * ld], o[ct]);
            }
        }
    };
    for (int kb = 0; kb < nlive; kb += BLK) {
        const int nk = min(BLK, nlive - kb);
        __syncthreads();
        stage_cache<BF16, PAGED>(KV, kc, spg, lgR, page_stride, kb, nk, dead, hdp, W, ld, tid);
        const int ids = cached_ids(kb, nk);
        __syncthreads();
        float p[4][4];
        if (wave_on) {
            cached_speakers(ids);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const f32x4 acc = dot_tile(kv_rows + 16 * jt * ld, qrow, ksteps);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = (vis.cached(i, kb + 16 * jt + 4 * lg + r) && (!SPK || m2f_spk_sees(spk_cls, spk4[jt], r, mine)))
                                        ? biased<BIAS>(acc[r] * scale, nslope, BIAS ? vis.cached_dist(i, kb + 16 * jt + 4 * lg + r) : 0) : -INFINITY;
                    p[jt][r] = (m_run == -INFINITY) ? 0.f : __expf(x - m_run) * inv;      // (no visible key: exp(-inf + inf) would be NaN)
                }
            }
        }
        __syncthreads();                                    // K consumed
        stage_cache<BF16, PAGED>(KV, vc, spg, lgR, page_stride, kb, nk, dead, hdp, W, ld, tid);
        __syncthreads();
        if (wave_on) pv(p, KV);
    }
    if (wave_on) {
        float p[4][4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 acc = dot_tile(own_rows + 16 * jt * ld, qrow, ksteps);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = (vis.own(i, 16 * jt + 4 * lg + r) && (!SPK || m2f_spk_sees(spk_cls, own4[jt], r, mine))) ? biased<BIAS>(acc[r] * scale, nslope, i - (16 * jt + 4 * lg + r)) : -INFINITY;
                p[jt][r] = (m_run == -INFINITY) ? 0.f : __expf(x - m_run) * inv;
            }
        }
        pv(p, Vs);
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
            if (ct >= CT) continue;
            const int c = 16 * ct + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = 16 * wv + 4 * lg + r;
                if (t < n_new && c < hd) {
                    const size_t idx = (row0 + t) * P.ldo + (size_t)h * hd + c;
                    P.out[idx] = o[ct][r];
                    if (out16) out16[idx] = m2f_bf16_bits(o[ct][r]);
                }
            }
        }
    }

    // ---- the new K / V rows into the cache: behind the workgroup's last cache read ------------------------------------------------
    __syncthreads();
    const int nst = min(n_new, C), t0 = n_new - nst;        // (n_new > C on a ring: the earlier rows would be overwritten in this launch)
    const int nch = hdp / EPL;                              // 16-byte chunks of a row; pad columns: the slab's zeros
    for (int e = tid; e < nst * nch; e += NTHR) {
        const int tr = e / nch, c = (e - tr * nch) * EPL, t = t0 + tr;
        const int pos = ab.ring ? (int)(((unsigned)n_old + (unsigned)t) % (unsigned)C) : n_old + t;
        const size_t o = PAGED ? m2f_stream_row_off(spg, lgR, page_stride, pos, hdp, c) : (size_t)pos * hdp + c;
        float kx[EPL], vx[EPL];                             // (already bf16 values in bf16 mode)
#pragma unroll
        for (int q = 0; q < EPL; ++q) { kx[q] = Ks[t * ld + c + q]; vx[q] = Vs[t * ld + c + q]; }
        R::store(kc + o, kx);
        R::store(vc + o, vx);
    }
}

template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(NTHR) void m2f_attn_stream_chunk_kernel(const AttnStreamBatch ab, const int T, const int* __restrict__ new_count) {
    attn_stream_chunk_body<BF16, false, BIAS, SPK>(ab, AttnStreamPaging{nullptr, 0, 0, 0, 0}, T, new_count);
}
template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(NTHR) void m2f_attn_stream_chunk_paged_kernel(const AttnStreamBatch ab, const AttnStreamPaging pg, const int T,
                                                                           const int* __restrict__ new_count) {
    attn_stream_chunk_body<BF16, true, BIAS, SPK>(ab, pg, T, new_count);
}

// len[s] += min(max(n_new[s], 0), T): the one launch that closes a prefill call
__global__ void m2f_stream_advance_n_kernel(int* len, const int* n_new, int S, int T) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) {
        const int n = min(max(n_new[s], 0), T);
        if (n) len[s] = len[s] + n;
    }
}

// ... of a stream with speaker heads: first the chunk's ids into the logical rows its utterances took - the rows the chunk kernel stored
// K / V to (a slot the chunk kernel left untouched keeps its bytes; of n > C new rows on a ring the last C) - one thread per slot, plain
// byte stores, behind every attention launch of the prefill call
__global__ void m2f_stream_advance_speakers_n_kernel(int* len, const int* n_new, int S, int T, uint8_t* spk_cache, const uint8_t* spk_new,
                                                     int C, int ring) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) {
        const int n = min(max(n_new[s], 0), T), n_old = len[s];
        const bool live = n > 0 && n_old >= 0 && (ring || (n_old <= C && n <= C - n_old));
        if (live)
            for (int t = n - min(n, C); t < n; ++t) {
                const int row = ring ? (int)(((unsigned)n_old + (unsigned)t) % (unsigned)C) : n_old + t;
                spk_cache[(size_t)s * C + row] = spk_new[(size_t)s * T + t];
            }
        if (n) len[s] = n_old + n;
    }
}

template <typename K, typename... Args>
hipError_t go(K kern, int blocks, size_t lds, hipStream_t stream, const Args&... args) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NTHR), lds, stream, args...);
    return hipGetLastError();
}

}  // namespace

hipError_t m2f_launch_attn_stream_chunk(AttnStreamBatch& ab, const AttnStreamPaging* paging, int T, const int* n_new, hipStream_t stream) {
    AttnStreamPaging pg = paging ? *paging : AttnStreamPaging{nullptr, 0, 0, 0, 0};
    int maxW = 0;
    const int blocks = n_new && T >= 1 && T <= M2F_ATTN_STREAM_MAX_CHUNK ? m2f_attn_stream_prepare(ab, paging ? &pg : nullptr, &maxW) : -1;
    if (blocks < 0 || !(ab.bias_gain >= 0.f) || ab.bias_gain > 3.0e38f) return hipErrorInvalidValue;
    const size_t lds = (size_t)4 * BLK * (maxW + 2) * sizeof(float);
    const bool spk = (ab.spk_same | ab.spk_other) != 0;
    if (spk && !m2f_attn_stream_speakers_ok(ab)) return hipErrorInvalidValue;
    return m2f_pick_bools([&](auto BF16, auto PAGED, auto BIAS, auto SPK) {       // one instantiation per combination of the four flags
        if constexpr (PAGED.value) return go(m2f_attn_stream_chunk_paged_kernel<BF16.value, BIAS.value, SPK.value>, blocks, lds, stream, ab, pg, T, n_new);
        else return go(m2f_attn_stream_chunk_kernel<BF16.value, BIAS.value, SPK.value>, blocks, lds, stream, ab, T, n_new);
    }, ab.bf16 != 0, paging != nullptr, ab.bias_gain != 0.f, spk);
}

hipError_t m2f_launch_stream_advance_n(int* len, const int* n_new, int S, int T, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_stream_advance_n_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, n_new, S, T);
    return hipGetLastError();
}

hipError_t m2f_launch_stream_advance_speakers_n(int* len, const int* n_new, int S, int T, uint8_t* spk_cache, const uint8_t* spk_new, int C,
                                                int ring, hipStream_t stream) {
    if (!len || !n_new || !spk_cache || !spk_new || S < 1 || T < 1 || T > M2F_ATTN_STREAM_MAX_CHUNK || C < 1 || C > M2F_ATTN_STREAM_MAX_C)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_stream_advance_speakers_n_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, n_new, S, T, spk_cache, spk_new, C, ring);
    return hipGetLastError();
}
