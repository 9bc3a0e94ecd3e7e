// Streaming ("decode") dialogue attention on gfx950: ONE new utterance per live dialogue against that dialogue's cached keys / values.
//
// The problem is (stream slot s, head h): the slot's new query row against the rows the slot has cached so far plus its new key row.
// Under a causal context band (past, 0) layer l's K and V rows of utterance j depend on utterances <= j only, so they are computed
// once, stored here, and never change; a step then costs one row per dialogue instead of the whole prefix.
//
// CACHE LAYOUT (per attention site, K and V alike), in one of two addressings:
//   dense   cache[S][H][C][hdp]        S slots, H heads, C rows of capacity
//   paged   pool[n_pages][H][R][hdp]   R = 16, 32 or 64 rows per page; logical cache row j of slot s lives at row j % R of page
//                                      table[s][j / R], table = int32 [S][ceil(C / R)].  Page ids are shared by every site of a
//                                      stream: page p is index p of every site's pool.
//   hdp = the head dim padded to a 16-byte multiple (m2f_stream_hdp): pad4(hd) floats (fp32 mode) or pad8(hd) bf16 values (bf16 mode).
//   A head's rows (dense) or its rows of one page (paged) are contiguous, every row starts 16-byte aligned, pad columns hold zeros.
//   m2f_attn_stream_cache_elems / m2f_attn_stream_pool_elems give the element counts.  Row r of a slot holds utterance r (plain cache,
//   len < C) or utterance u with u % C == r (ring: a window of past = C - 1 utterances; the row of the utterance that just left the
//   window is the one the new utterance overwrites).  The number of live rows comes from len[s] alone, so stale rows behind a reset are
//   never read.
//
// One wavefront per (s, h): byte-stream work (every cached row is read exactly once, with 16-byte loads straight into VGPRs), no MFMA.
// A row is spread over CH = 2^k lanes (4 floats / 8 bf16 each; lanes past the row's end hold zeros in registers, no divergent tail),
// 64 / CH rows per pass.  Pass 1: scores into LDS (fp32 product, then * 1/sqrt(hd), as attention.hip); softmax: max-subtracted __expf
// in fp32 over the <= 512 scores; pass 2: P V with per-lane fp32 accumulators, folded across the row groups by a fixed xor butterfly.
// No atomics, a fixed summation order: the same bits on every run.  The slot's own K / V row is taken from LDS, where the new rows are
// staged (rounded once in bf16 mode: what the cache then holds), never read back from the cache row the same wave has just written.
// len[] is NOT advanced here: every site of a step reads the same count, m2f_launch_stream_advance closes the step.
//
// The two addressings are ONE kernel body (attn_stream_body<BF16, PAGED>): work split, row order, arithmetic and summation order are
// one text, so the paged form gives the dense form's bits.  Behind PAGED stand only the fetch of the slot's page ids into LDS
// (attn_stream_rows.h: the entries of pages that hold a live row or take the new one, e < ceil(min(len + 1, C) / R)), the base pointer
// of a head's rows and the offset of row j.
//
// WEIGHTS (a third flag of the body, its own instantiations; the others are the text they were): behind the softmax the wave also stores
// its row of probabilities sc[j] * inv - the pre-normalised exponentials times the reciprocal the output row is scaled by - to
// ww.w[problem][s][h][0 .. C) in LOGICAL order: column t is the t-th oldest live utterance, the last live column the utterance that
// has just arrived (a ring: utterance u sits in row u % C, which is undone here; the page table never enters: the order is logical).
// Columns behind the live count are zeros, an inactive slot gets a row of zeros.  Ordinary per-lane vector stores, 64 consecutive
// floats per instruction.
//
// BIAS (a fourth flag, its own instantiations again): the launch has a distance-decay bias (ops.h, m2f_attn_bias_slope; AttnStreamBatch::
// bias_gain).  The new utterance is utterance n_old; cache row j holds the utterance at distance n_old - j (plain cache) or
// (pos - j + C) % C (ring), and -slope * distance is added to the scaled score where it is written - an explicit fma, one rounding
// rule with the dialogue kernels.  The cached rows do not depend on it.
//
// SPK (a fifth flag, its own instantiations again): the launch has speaker heads (ops.h, m2f_attn_speaker_class; AttnStreamBatch::spk_cache /
// spk_new).  The wave reads the slot's cached speaker bytes ONCE, lane = logical row, 64 consecutive bytes per load and up to 512 B in
// all, into LDS beside the new rows; the new utterance's id is the step input spk_new[s] and the cached byte of the row it takes (a
// ring: the utterance that just left the window) is never read.  Pass 1 writes -inf for a row its head's class hides.  The new row is
// visible to a same-speaker head and to an untouched one, but an other-speaker head with no other speaker cached sees NO row: there
// the maximum is -inf, and the SPK form writes zero exponentials and scales by 0 - a zero output row, a zero weights row - where the
// text without the flag may divide, its sum being >= 1.  The bytes are written by m2f_launch_stream_advance_speakers, behind every
// attention launch of the step.
#include "common.h"
#include "ops.h"
#include "attn_stream_rows.h"

namespace {

template <bool BF16, bool PAGED, bool WEIGHTS, bool BIAS, bool SPK = false>
__device__ __forceinline__ void attn_stream_body(const AttnStreamBatch& ab, const AttnStreamPaging& pg, const AttnStreamWeights& ww) {
    typedef Row<BF16> R;
    typedef typename R::elem_t elem_t;
    constexpr int EPL = R::EPL;
    constexpr int U = 4;                          // passes in flight: their loads are issued together
    __shared__ float sq[128], sk[128], sv[128];   // the slot's new rows of this head, zero behind hd (bf16 mode: rounded)
    __shared__ float sc[M2F_ATTN_STREAM_MAX_C];   // scores, then the unnormalised probabilities
    __shared__ int spg[32];                       // paged: the slot's page ids, entry e = logical rows e*R .. e*R + R - 1
    __shared__ uint8_t sspk[SPK ? M2F_ATTN_STREAM_MAX_C : 4];     // SPK: the speaker ids of the slot's logical cache rows

    const int blk = blockIdx.x, lane = threadIdx.x;
    int pi = 0;
    while (pi + 1 < ab.count && blk >= ab.bb[pi + 1]) ++pi;
    const AttnStreamProblem& P = ab.pr[pi];
    const int local = blk - ab.bb[pi];
    const int s = local / P.H, h = local - s * P.H;
    const int hd = P.hd, C = ab.C;
    const int hdp = m2f_stream_hdp(hd, BF16);
    float* orow = P.out + (size_t)s * P.ldo + (size_t)h * hd;
    uint16_t* orow16 = m2f_shadow_of(ab.sh, orow);

    const int n_old = ab.len[s];
    const bool live = ab.active[s] != 0 && n_old >= 0 && (ab.ring || n_old < C);
    if (!live) {                                  // inactive slot: a zero output row, cache and len untouched
        for (int i = lane; i < hd; i += 64) {
            orow[i] = 0.f;
            if (orow16) orow16[i] = 0;
        }
        if constexpr (WEIGHTS) {
            float* wrow = ww.w[pi] + ((size_t)s * P.H + h) * (size_t)C;
            for (int t = lane; t < C; t += 64) wrow[t] = 0.f;
        }
        return;
    }
    const int pos = ab.ring ? n_old % C : n_old;              // the row the new utterance takes
    const int nslots = n_old + 1 < C ? n_old + 1 : C;         // live rows, the new one included
    const int lgR = PAGED ? pg.lgR : 0;

    if (PAGED) m2f_stream_page_ids(spg, pg, s, nslots, lane);
    int spk_cls = M2F_SPK_NONE, mine = 0;         // SPK: the head's class (uniform per wave), the new utterance's speaker
    if constexpr (SPK) {
        spk_cls = m2f_attn_speaker_class(h, ab.spk_same, ab.spk_other);
        mine = ab.spk_new[s];
        const uint8_t* crow = ab.spk_cache + (size_t)s * C;
        for (int j = lane; j < nslots; j += 64) sspk[j] = crow[j];       // (nslots <= C <= 512: at most eight coalesced byte loads)
    }
    {   // the new rows -> LDS
        const float* qrow = P.q + (size_t)s * P.ldq + (size_t)h * hd;
        const float* krow = P.k + (size_t)s * P.ldk + (size_t)h * hd;
        const float* vrow = P.v + (size_t)s * P.ldv + (size_t)h * hd;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int i = lane + 64 * t;
            float a = 0.f, b = 0.f, c = 0.f;
            if (i < hd) { a = qrow[i]; b = krow[i]; c = vrow[i]; }
            if (BF16) { a = m2f_bf16_to_f32(m2f_bf16_bits(a)); b = m2f_bf16_to_f32(m2f_bf16_bits(b)); c = m2f_bf16_to_f32(m2f_bf16_bits(c)); }
            sq[i] = a; sk[i] = b; sv[i] = c;
        }
    }
    __syncthreads();

    const int nch = hdp / EPL;                    // 16-byte chunks per row
    int CH = 1, lg = 0;
    while (CH < nch) { CH <<= 1; ++lg; }          // lanes per row (<= 32: hd <= 128)
    const int RPW = 64 >> lg;                     // rows per pass
    const int r = lane >> lg, c = lane & (CH - 1);
    const bool cact = c < nch;
    const int e0 = c * EPL;                       // (< 128 for every lane: CH * EPL <= 128)

    // this lane's chunk of row 0 of the head: of the slot's cache (dense) or of page 0 (paged), and from there to row j
    const size_t page_stride = (size_t)P.H * (size_t)(hdp << lgR);       // paged: elements of one page, all heads
    const size_t head0 = PAGED ? (size_t)h * (size_t)(hdp << lgR) + e0 : ((size_t)s * P.H + h) * (size_t)C * hdp + e0;
    elem_t* kc = static_cast<elem_t*>(P.kcache) + head0;
    elem_t* vc = static_cast<elem_t*>(P.vcache) + head0;
    auto row_off = [&](int j) { return PAGED ? m2f_stream_row_off(spg, lgR, page_stride, j, hdp) : (size_t)j * hdp; };
    if (r == 0 && cact) {                         // the new K / V rows into the cache (vector stores; pad columns: zeros)
        float kx[EPL], vx[EPL];
#pragma unroll
        for (int i = 0; i < EPL; ++i) { kx[i] = sk[e0 + i]; vx[i] = sv[e0 + i]; }
        const size_t o = row_off(pos);
        R::store(kc + o, kx);
        R::store(vc + o, vx);
    }

    float qx[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) qx[i] = sq[e0 + i];
    const float scale = 1.0f / sqrtf((float)hd);
    float nslope = 0.f;                           // BIAS: minus the head's slope
    if constexpr (BIAS) nslope = -m2f_attn_bias_slope(h, P.H, ab.bias_gain);

    // ---- pass 1: scores ---------------------------------------------------------------------------------------------------------
    for (int j0 = 0; j0 < nslots; j0 += RPW * U) {
        float kx[U][EPL];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * RPW + r;
#pragma unroll
            for (int i = 0; i < EPL; ++i) kx[u][i] = 0.f;
            if (cact && j < nslots) {
                if (j != pos) R::load(kc + row_off(j), kx[u]);
                else {
#pragma unroll
                    for (int i = 0; i < EPL; ++i) kx[u][i] = sk[e0 + i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * RPW + r;
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < EPL; ++i) d = fmaf(qx[i], kx[u][i], d);
            for (int o = CH >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
            bool hide = false;                                                  // SPK: a row the head's class hides gets -inf
            if constexpr (SPK) {
                const bool eq = j == pos || (j < nslots && sspk[j] == mine);    // (the new row carries `mine`; its cached byte is stale)
                hide = spk_cls != M2F_SPK_NONE && eq != (spk_cls == M2F_SPK_SAME);
            }
            if constexpr (BIAS) {
                int dist = pos - j;                                             // plain cache: pos = n_old >= j; ring: (pos - j + C) % C
                if (dist < 0) dist += C;                                        // (0 <= pos, j < C: one wrap at most, no division)
                if (c == 0 && j < nslots) sc[j] = hide ? -INFINITY : __fmaf_rn(nslope, (float)dist, d * scale);
            } else {
                if (c == 0 && j < nslots) sc[j] = hide ? -INFINITY : d * scale;
            }
        }
    }
    __syncthreads();

    // ---- softmax over the live rows (fp32, max-subtracted) ------------------------------------------------------------------------
    float m = -INFINITY;
    for (int j = lane; j < nslots; j += 64) m = fmaxf(m, sc[j]);
    m = m2f_wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nslots; j += 64) {
        const float e = (SPK && m == -INFINITY) ? 0.f : __expf(sc[j] - m);       // (SPK: no visible row - not exp(-inf + inf))
        sc[j] = e;
        sum += e;
    }
    sum = m2f_wave_sum(sum);
    const float inv = (SPK && !(sum > 0.f)) ? 0.f : 1.0f / sum;      // (sum >= 1: the row of the maximum contributes exp(0); SPK: or no row is visible)
    __syncthreads();
    if constexpr (WEIGHTS) {                      // the row of probabilities, oldest live utterance first
        float* wrow = ww.w[pi] + ((size_t)s * P.H + h) * (size_t)C;
        const int first = n_old + 1 - nslots;     // utterance index of column 0 (plain cache: 0, row t holds utterance t)
        for (int t = lane; t < C; t += 64) wrow[t] = t < nslots ? sc[ab.ring ? (first + t) % C : t] * inv : 0.f;
    }

    // ---- pass 2: P V ---------------------------------------------------------------------------------------------------------------
    float acc[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < nslots; j0 += RPW * U) {
        float vx[U][EPL], p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * RPW + r;
#pragma unroll
            for (int i = 0; i < EPL; ++i) vx[u][i] = 0.f;
            p[u] = 0.f;
            if (cact && j < nslots) {
                p[u] = sc[j];
                if (j != pos) R::load(vc + row_off(j), vx[u]);
                else {
#pragma unroll
                    for (int i = 0; i < EPL; ++i) vx[u][i] = sv[e0 + i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < EPL; ++i) acc[i] = fmaf(p[u], vx[u][i], acc[i]);
    }
    for (int o = CH; o < 64; o <<= 1) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
    }
    if (r == 0 && cact) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            if (e0 + i < hd) {
                const float o = acc[i] * inv;
                orow[e0 + i] = o;
                if (orow16) orow16[e0 + i] = m2f_bf16_bits(o);
            }
        }
    }
}

template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(64) void m2f_attn_stream_kernel(const AttnStreamBatch ab) {
    attn_stream_body<BF16, false, false, BIAS, SPK>(ab, AttnStreamPaging{nullptr, 0, 0, 0, 0}, AttnStreamWeights{{nullptr}});
}
template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(64) void m2f_attn_stream_paged_kernel(const AttnStreamBatch ab, const AttnStreamPaging pg) {
    attn_stream_body<BF16, true, false, BIAS, SPK>(ab, pg, AttnStreamWeights{{nullptr}});
}
template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(64) void m2f_attn_stream_weights_kernel(const AttnStreamBatch ab, const AttnStreamWeights ww) {
    attn_stream_body<BF16, false, true, BIAS, SPK>(ab, AttnStreamPaging{nullptr, 0, 0, 0, 0}, ww);
}
template <bool BF16, bool BIAS = false, bool SPK = false>
__global__ __launch_bounds__(64) void m2f_attn_stream_paged_weights_kernel(const AttnStreamBatch ab, const AttnStreamPaging pg, const AttnStreamWeights ww) {
    attn_stream_body<BF16, true, true, BIAS, SPK>(ab, pg, ww);
}

// len[s] += active[s]: the one launch that closes a step
__global__ void m2f_stream_advance_kernel(int* len, const uint8_t* active, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && active[s]) len[s] = len[s] + 1;
}
// ... of a stream with speaker heads: first the new utterance's id into the logical row it took (ring: row len % C, the byte of the
// utterance that just left the window; every attention launch of the step has read the old row set - they are earlier in the stream)
__global__ void m2f_stream_advance_speakers_kernel(int* len, const uint8_t* active, int S, uint8_t* spk_cache, const uint8_t* spk_new,
                                                   int C, int ring) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && active[s]) {
        const int n = len[s];
        const int row = ring ? (n >= 0 ? n % C : -1) : n;
        if (row >= 0 && row < C) spk_cache[(size_t)s * C + row] = spk_new[s];
        len[s] = n + 1;
    }
}
// len[s] = 0 for the slots of the mask (null: every slot)
__global__ void m2f_stream_reset_kernel(int* len, const uint8_t* mask, int S) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S && (!mask || mask[s])) len[s] = 0;
}

template <typename K, typename... Args>
hipError_t go(K kern, int blocks, hipStream_t stream, const Args&... args) {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace

size_t m2f_attn_stream_cache_elems(int S, int H, int hd, int C, int bf16) { return (size_t)S * H * C * m2f_stream_hdp(hd, bf16 != 0); }
size_t m2f_attn_stream_pool_elems(int n_pages, int H, int hd, int R, int bf16) { return (size_t)n_pages * H * R * m2f_stream_hdp(hd, bf16 != 0); }

// What every paged launcher refuses before anything is launched; fills pg.lgR.
bool m2f_attn_stream_paging_ok(const AttnStreamBatch& ab, AttnStreamPaging& pg) {
    if (pg.R != 16 && pg.R != 32 && pg.R != 64) return false;
    if (!pg.table || (reinterpret_cast<uintptr_t>(pg.table) & 3) || pg.n_pages < 1) return false;
    if (ab.C < 1 || ab.C > M2F_ATTN_STREAM_MAX_C || pg.tw != (ab.C + pg.R - 1) / pg.R) return false;
    pg.lgR = pg.R == 16 ? 4 : pg.R == 32 ? 5 : 6;
    return true;
}

// What the step and the chunk launcher refuse, dense or paged (pg: null for dense; a copy, lgR filled, goes to the kernel), and the
// launch geometry: block_begin / bb[] of every problem.  -> workgroups, or -1; *maxW: the widest head dim padded to 16.
int m2f_attn_stream_prepare(AttnStreamBatch& ab, AttnStreamPaging* pg, int* maxW) {
    if (ab.count < 1 || ab.count > M2F_ATTN_MAX_PROBLEMS || ab.S < 1 || ab.C < 1 || ab.C > M2F_ATTN_STREAM_MAX_C || !ab.len) return -1;
    if (pg && !m2f_attn_stream_paging_ok(ab, *pg)) return -1;
    int blocks = 0, w = 0;
    for (int i = 0; i < M2F_ATTN_MAX_PROBLEMS; ++i) ab.bb[i] = 0x7fffffff;
    for (int i = 0; i < ab.count; ++i) {
        AttnStreamProblem& p = ab.pr[i];
        if (p.H < 1 || p.hd < 1 || p.hd > 128 || !p.q || !p.k || !p.v || !p.out || !p.kcache || !p.vcache) return -1;
        if ((reinterpret_cast<uintptr_t>(p.kcache) & 15) || (reinterpret_cast<uintptr_t>(p.vcache) & 15)) return -1;
        p.block_begin = blocks;
        ab.bb[i] = blocks;
        blocks += ab.S * p.H;
        w = w > ((p.hd + 15) & ~15) ? w : (p.hd + 15) & ~15;
    }
    if (maxW) *maxW = w;
    return blocks;
}

hipError_t m2f_launch_attn_stream(AttnStreamBatch& ab, const AttnStreamPaging* paging, hipStream_t stream, const AttnStreamWeights* weights) {
    AttnStreamPaging pg = paging ? *paging : AttnStreamPaging{nullptr, 0, 0, 0, 0};
    const int blocks = ab.active ? m2f_attn_stream_prepare(ab, paging ? &pg : nullptr, nullptr) : -1;
    if (blocks < 0 || !(ab.bias_gain >= 0.f) || ab.bias_gain > 3.0e38f) return hipErrorInvalidValue;
    if (weights)
        for (int i = 0; i < ab.count; ++i)
            if (!weights->w[i] || (reinterpret_cast<uintptr_t>(weights->w[i]) & 3)) return hipErrorInvalidValue;
    const bool spk = (ab.spk_same | ab.spk_other) != 0;
    if (spk && !m2f_attn_stream_speakers_ok(ab)) return hipErrorInvalidValue;
    const AttnStreamWeights ww = weights ? *weights : AttnStreamWeights{{nullptr}};
    // one instantiation per combination of the five flags; PAGED / WEIGHTS also choose the wrapper, whose argument list they shape
    return m2f_pick_bools([&](auto BF16, auto PAGED, auto WEIGHTS, auto BIAS, auto SPK) {
        constexpr bool b16 = BF16.value, paged = PAGED.value, wts = WEIGHTS.value, bias = BIAS.value, sp = SPK.value;
        if constexpr (paged && wts) return go(m2f_attn_stream_paged_weights_kernel<b16, bias, sp>, blocks, stream, ab, pg, ww);
        else if constexpr (wts) return go(m2f_attn_stream_weights_kernel<b16, bias, sp>, blocks, stream, ab, ww);
        else if constexpr (paged) return go(m2f_attn_stream_paged_kernel<b16, bias, sp>, blocks, stream, ab, pg);
        else return go(m2f_attn_stream_kernel<b16, bias, sp>, blocks, stream, ab);
    }, ab.bf16 != 0, paging != nullptr, weights != nullptr, ab.bias_gain != 0.f, spk);
}

hipError_t m2f_launch_stream_advance(int* len, const uint8_t* active, int S, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_stream_advance_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, active, S);
    return hipGetLastError();
}

hipError_t m2f_launch_stream_advance_speakers(int* len, const uint8_t* active, int S, uint8_t* spk_cache, const uint8_t* spk_new, int C,
                                              int ring, hipStream_t stream) {
    if (!len || !active || !spk_cache || !spk_new || S < 1 || C < 1 || C > M2F_ATTN_STREAM_MAX_C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(m2f_stream_advance_speakers_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, active, S, spk_cache, spk_new, C, ring);
    return hipGetLastError();
}

hipError_t m2f_launch_stream_reset(int* len, const uint8_t* mask, int S, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_stream_reset_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, len, mask, S);
    return hipGetLastError();
}
