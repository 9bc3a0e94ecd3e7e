// Attention maps on gfx950: the P^T that the dialogue attention forwards save (attention.hip, attention_dlong.hip: [B*H, Lp, Lp] per site,
// pre-dropout, consecutive QUERIES in memory) -> what nn.MultiheadAttention(need_weights=True) returns: [B, H, L, L] per head or the
// head average [B, L, L], consecutive KEYS in memory.  One launch serves every listed site (a by-value site table, as stream_cache.hip's).
//
// A workgroup of 256 lanes owns one 32 x 32 tile (queries i0 .. i0 + 31, keys j0 .. j0 + 31) of one (site, dialogue[, head]):
//   load   lane t reads P^T[j0 + (t >> 5) + 8 r][i0 + (t & 31)], r = 0 .. 3: 32 consecutive floats per row of P^T, 128-byte segments;
//          the averaged form walks h = 0 .. H - 1 in that order with one fp32 accumulator per element (acc = P_0; acc = acc + P_h),
//          then acc * inv_h with inv_h = 1.0f / H from the host: torch's average_attn_weights with a fixed order, no atomics, the
//          same bits on every run.  The per-head form moves the value itself.
//   turn   through an LDS tile [32][33] floats with 4-byte accesses (ds_write_b32 / ds_read_b32 bank = word address mod 32, conflicts
//          counted per 32-lane half): the write of a half has one key row and 32 consecutive queries (word 33 j + i: 32 banks), the
//          read-back has bank (j + i) mod 32 with either (j = 4 a + c, i = i1 + b: a < 8, b < 4, the 16-byte form) or (j = lane, i
//          fixed): all distinct.  No conflict on either side.
//   store  16-byte stores of four consecutive keys where L % 4 == 0 (every output row then starts 16-byte aligned), else 4-byte stores
//          of 32 consecutive keys.
// WHAT IS READ.  Element (i, j) is loaded only if i < n and j < n (n: the dialogue's length in a packed launch, L in a padded one), key
// j is not padded and the context band admits the pair; every other element of the [L, L] map is written as exactly 0.  This is not
// cosmetic: under a band the long-dialogue forward skips hidden 64-row block pairs and leaves in them what the buffer held, and
// neither long-dialogue kernel writes the tile rows behind a short dialogue.  No byte the forward did not write is trusted.
// Pad-query rows of a padded launch keep their softmax numbers (torch has numbers there too); a row that sees no key is zeros.
#include "common.h"
#include "ops.h"

// (as attention.hip: the averaged form's add-then-scale must stay two rounded operations)
#pragma clang fp contract(off)

namespace {

constexpr int TW = 32;                            // tile edge
constexpr int TS = TW + 1;                        // LDS row stride in floats

__global__ __launch_bounds__(256) void m2f_attn_weights_kernel(const AttnWeightsBatch wb) {
    __shared__ float tile[TW * TS];               // tile[j][i]

    const int blk = blockIdx.x, t = threadIdx.x;
    int si = 0;
    while (si + 1 < wb.count && blk >= wb.sb[si + 1]) ++si;
    const AttnWeightsSite& st = wb.site[si];
    const int L = wb.L, H = st.H;
    const int Lp = 16 * ((L + 15) >> 4), nt = (L + TW - 1) / TW;
    int local = blk - wb.sb[si];
    const int tj = local % nt; local /= nt;
    const int ti = local % nt; local /= nt;       // local: the dialogue, or (dialogue, head)
    const int b = wb.per_head ? local / H : local, h0 = wb.per_head ? local - b * H : 0, nh = wb.per_head ? 1 : H;
    int n = L;
    if (wb.cu) { n = wb.cu[b + 1] - wb.cu[b]; n = n < 0 ? 0 : (n > L ? L : n); }

    {
        const int i = TW * ti + (t & 31);
        float acc[4];
        bool see[4];
        int j[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            j[r] = TW * tj + (t >> 5) + 8 * r;
            bool ok = i < n && j[r] < n;
            if (ok && !wb.cu && wb.key_pad) ok = wb.key_pad[(size_t)b * L + j[r]] == 0;
            // the band: the two compares of m2f_attn_band_bits
            if (wb.band_past && j[r] < i - (wb.band_past - 1)) ok = false;
            if (wb.band_future && j[r] > i + (wb.band_future - 1)) ok = false;
            see[r] = ok;
            acc[r] = 0.f;
        }
        const float* p = st.probs + (size_t)(b * H + h0) * Lp * Lp + i;
        for (int h = 0; h < nh; ++h, p += (size_t)Lp * Lp) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = see[r] ? p[(size_t)j[r] * Lp] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h == 0 ? v[r] : acc[r] + v[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[((t >> 5) + 8 * r) * TS + (t & 31)] = wb.per_head ? acc[r] : acc[r] * st.inv_h;
    }
    __syncthreads();

    float* out = st.out + (size_t)local * L * L;  // (local = b * H + h per head, b averaged: the map's index in both layouts)
    if (wb.vec) {
        const int il = t >> 3, jl = (t & 7) * 4;
        const int i = TW * ti + il, j = TW * tj + jl;
        if (i < L && j < L) {                     // (L % 4 == 0: j + 3 < L)
            const f32x4 v = {tile[jl * TS + il], tile[(jl + 1) * TS + il], tile[(jl + 2) * TS + il], tile[(jl + 3) * TS + il]};
            *reinterpret_cast<f32x4*>(out + (size_t)i * L + j) = v;
        }
    } else {
        const int jl = t & 31, j = TW * tj + jl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = (t >> 5) + 8 * r, i = TW * ti + il;
            if (i < L && j < L) out[(size_t)i * L + j] = tile[jl * TS + il];
        }
    }
}

// ROWS mode: site rows [B][H][L] as the weights-emitting stream step stores them (attention_stream.hip), keys already consecutive ->
// [B][L] by the same rule (acc = P_0; acc = acc + P_h; acc * inv_h), or a copy [B][H][L].  One lane per output element.
__global__ __launch_bounds__(256) void m2f_attn_weight_rows_kernel(const AttnWeightsBatch wb) {
    const int blk = blockIdx.x;
    int si = 0;
    while (si + 1 < wb.count && blk >= wb.sb[si + 1]) ++si;
    const AttnWeightsSite& st = wb.site[si];
    const int L = wb.L, H = st.H;
    const long long e = (long long)(blk - wb.sb[si]) * 256 + threadIdx.x;
    if (wb.per_head) {
        if (e < (long long)wb.B * H * L) st.out[e] = st.probs[e];
        return;
    }
    if (e >= (long long)wb.B * L) return;
    const long long b = e / L, c = e - b * L;
    const float* p = st.probs + (size_t)b * H * L + c;
    float acc = p[0];
    for (int h = 1; h < H; ++h) acc = acc + p[(size_t)h * L];
    st.out[e] = acc * st.inv_h;
}

}  // namespace

hipError_t m2f_launch_attn_weight_rows(AttnWeightsBatch& wb, hipStream_t stream) {
    if (wb.count < 1 || wb.count > M2F_ATTN_WEIGHTS_MAX_SITES || wb.B < 1 || wb.L < 1) return hipErrorInvalidValue;
    long long blocks = 0;
    for (int i = 0; i < M2F_ATTN_WEIGHTS_MAX_SITES; ++i) wb.sb[i] = 0x7fffffff;
    for (int i = 0; i < wb.count; ++i) {
        const AttnWeightsSite& s = wb.site[i];
        if (!s.probs || !s.out || s.H < 1) return hipErrorInvalidValue;
        wb.sb[i] = (int)blocks;
        blocks += ((long long)wb.B * (wb.per_head ? s.H : 1) * wb.L + 255) / 256;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    }
    wb.per_head = wb.per_head != 0;
    hipLaunchKernelGGL(m2f_attn_weight_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, wb);
    return hipGetLastError();
}

hipError_t m2f_launch_attn_weights(AttnWeightsBatch& wb, hipStream_t stream) {
    if (wb.count < 1 || wb.count > M2F_ATTN_WEIGHTS_MAX_SITES || wb.B < 1 || wb.L < 1 || wb.L > M2F_ATTN_DLONG_MAX_L) return hipErrorInvalidValue;
    if (wb.band_past < 0 || wb.band_future < 0) return hipErrorInvalidValue;
    const long long nt = (wb.L + TW - 1) / TW;
    long long blocks = 0;
    bool vec = wb.L % 4 == 0;
    for (int i = 0; i < M2F_ATTN_WEIGHTS_MAX_SITES; ++i) wb.sb[i] = 0x7fffffff;
    for (int i = 0; i < wb.count; ++i) {
        const AttnWeightsSite& s = wb.site[i];
        if (!s.probs || !s.out || s.H < 1 || (reinterpret_cast<uintptr_t>(s.out) & 3)) return hipErrorInvalidValue;
        if (reinterpret_cast<uintptr_t>(s.out) & 15) vec = false;
        wb.sb[i] = (int)blocks;
        blocks += (long long)wb.B * (wb.per_head ? s.H : 1) * nt * nt;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    }
    wb.vec = vec;
    wb.per_head = wb.per_head != 0;
    hipLaunchKernelGGL(m2f_attn_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, wb);
    return hipGetLastError();
}
