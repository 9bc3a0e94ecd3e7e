// Supervised contrastive criterion (Khosla et al. 2020) over the rows of a feature matrix, forward and backward, exact fp32 on gfx950.
//
// Definition (SupconArgs, ops.h).  h_i = row i of feat, y_i its label.  V = rows with 0 <= y_i < C and ||h_i|| > 0 (the norm as this
// file computes it: sqrtf of the fp32 sum of squares).  z_i = h_i / ||h_i||, s_ia = (z_i . z_a) / tau, A(i) = V \ {i},
// P(i) = {a in A(i): y_a = y_i}, n_i = |P(i)|:
//   l_i  = lse_{a in A(i)} s_ia - (1 / n_i) sum_{p in P(i)} s_ip        for i in V with n_i > 0, else l_i = 0 (SELECTED)
//   c_i  = lambda * w_{y_i} * [i in V and n_i > 0]
//   dz_i = (1 / tau) sum_{a in A(i)} [c_i (p_ia - m_ia / n_i) + c_a (p_ai - m_ia / n_a)] z_a      p_ia = exp(s_ia - lse_i), m_ia = [y_i = y_a]
//   dh_i = (dz_i - (dz_i . z_i) z_i) / ||h_i||                          zeros outside V
// s is symmetric, so the row's share as somebody else's key needs only that key's lse, n and c: the backward recomputes s per tile and
// owns every output row in one workgroup - no [N, N] buffer, no atomics.
//
// Launches (m2f_launch_supcon, one stream, in order):
//   prep   one wave per row: norm, validity, z_i (divided, as the definition reads) into a zero-padded copy Z [Np, Dp] of the
//          workspace (Np, Dp: N, D rounded up to 64) - every tile below is full, no bounds test inside an MFMA loop
//   fwd    one workgroup per (64 anchors, group of key blocks; one block per group up to 1,024 rows): per 64 keys S = Z_a Z_k^T on
//          v_mfma_f32_16x16x4_f32, K streamed through LDS 32 floats at a time (register-staged one chunk ahead); a row's (max, sum exp,
//          sum of positives, count) kept online over the group's blocks, then part[group][row]
//   rows   one lane per row: the groups' partials merged IN GROUP ORDER (max first, then the rescaled sums) -> lse, n, l, w l
//          (row_terms), 1 / n and c for the backward, and the numerator of loss_terms
//   bwd    one workgroup per (64 anchors, group of pairs of key blocks; one pair per group up to 1,024 rows): per pair S again, the
//          coefficient tiles G into LDS, then dz += G Z_k, 64 output columns at a time -> dzp[group][row]
//   dfeat  one wave per row: the groups' partial dz summed IN GROUP ORDER, the projection off z_i and the division by ||h_i||
// The tile sizes and the group counts are constants of this file, the grids follow from N alone: a launch has no shape to choose, every
// sum has one order, two runs give the same bits.
#include "common.h"
#include "ops.h"

#include <algorithm>

namespace {

constexpr int SC_T = 64;         // anchors / keys per tile
constexpr int SC_KC = 32;        // K floats per staged chunk of the S product
constexpr int SC_LDS = SC_KC + 4;    // its LDS row stride: 4 mod 32, the 16 rows x 4 k of a fragment read hit 64 banks
constexpr int SC_KG = 2;         // key blocks per backward workgroup
constexpr int SC_LDG = SC_T + 4;     // row stride of a coefficient tile in LDS (read as the A operand: as SC_LDS)
constexpr int SC_NC = 64;        // output columns per step of the G Z product
constexpr int SC_LDZ = SC_NC + 16;   // row stride of its key slab (read as the B operand: 4 k rows x 16 columns, 16 mod 64)

__device__ __forceinline__ f32x4 sc_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc[j][r] = sum_k Z[a0 + 16 wave + 4 (lane >> 4) + r][k] * Z[k0 + 16 j + (lane & 15)][k] over all Dp columns.  As, Bs: SC_T * SC_LDS floats each.
__device__ __forceinline__ void sc_s_tile(const float* __restrict__ Z, int Dp, int a0, int k0, float* __restrict__ As,
                                          float* __restrict__ Bs, f32x4 (&acc)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15, lq = lane >> 4;
    const int lr = tid >> 3, lc = (tid & 7) * 4;            // this thread stages rows lr and lr + 32, columns lc .. lc + 3 of both chunks
    const float* ga = Z + (size_t)(a0 + lr) * Dp + lc;
    const float* gb = Z + (size_t)(k0 + lr) * Dp + lc;
    const size_t half = (size_t)32 * Dp;
    f32x4 ra0 = *reinterpret_cast<const f32x4*>(ga), ra1 = *reinterpret_cast<const f32x4*>(ga + half);
    f32x4 rb0 = *reinterpret_cast<const f32x4*>(gb), rb1 = *reinterpret_cast<const f32x4*>(gb + half);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < Dp; kc += SC_KC) {
        __syncthreads();                                    // (the previous chunk's - or the caller's - reads of the slabs are done)
        *reinterpret_cast<f32x4*>(As + lr * SC_LDS + lc) = ra0;
        *reinterpret_cast<f32x4*>(As + (lr + 32) * SC_LDS + lc) = ra1;
        *reinterpret_cast<f32x4*>(Bs + lr * SC_LDS + lc) = rb0;
        *reinterpret_cast<f32x4*>(Bs + (lr + 32) * SC_LDS + lc) = rb1;
        __syncthreads();
        if (kc + SC_KC < Dp) {
            ra0 = *reinterpret_cast<const f32x4*>(ga + kc + SC_KC); ra1 = *reinterpret_cast<const f32x4*>(ga + half + kc + SC_KC);
            rb0 = *reinterpret_cast<const f32x4*>(gb + kc + SC_KC); rb1 = *reinterpret_cast<const f32x4*>(gb + half + kc + SC_KC);
        }
        const float* ar = As + (16 * wv + l16) * SC_LDS + lq;
        const float* br = Bs + l16 * SC_LDS + lq;
#pragma unroll
        for (int k4 = 0; k4 < SC_KC; k4 += 4) {
            const float a = ar[k4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = sc_mfma(a, br[16 * j * SC_LDS + k4], acc[j]);
        }
    }
}

// sum / max over the 16 lanes that share an accumulator row (lane & 15), fixed order; every lane of the group gets the result
__device__ __forceinline__ float sc_row_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float sc_row_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per row of the padded copy.  Rows past N and columns past D are zeros; so is every row outside V, and its ylab is -1.
__global__ __launch_bounds__(256) void m2f_supcon_prep_kernel(const float* __restrict__ feat, int N, int D, int ld,
                                                              const int64_t* __restrict__ labels, int C, int Dp,
                                                              float* __restrict__ Z, float* __restrict__ rinv, int* __restrict__ ylab) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);      // (the grid covers Np rows exactly)
    const bool row = r < N;
    float ss = 0.f;
    if (row)
        for (int c = lane; c < D; c += 64) { const float v = feat[(size_t)r * ld + c]; ss += v * v; }
    ss = m2f_wave_sum(ss);
    const float norm = sqrtf(ss);
    const int64_t y = row ? labels[r] : -1;
    const bool valid = row && y >= 0 && y < C && norm > 0.f;
    for (int c = lane; c < Dp; c += 64)
        Z[(size_t)r * Dp + c] = (valid && c < D) ? feat[(size_t)r * ld + c] / norm : 0.f;
    if (lane == 0) { rinv[r] = valid ? 1.0f / norm : 0.f; ylab[r] = valid ? (int)y : -1; }
}

// Workgroup (anchor block, key group g): the group's key blocks g * per .. in order, a row's (max, sum exp, sum of positives, count) kept
// online in registers (the running sum rescaled when the max moves), then part[g][row].
__global__ __launch_bounds__(256) void m2f_supcon_fwd_kernel(const float* __restrict__ Z, const int* __restrict__ ylab,
                                                             const float* __restrict__ hyper, int Np, int Dp, int nkb, int per,
                                                             float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[SC_T * SC_LDS];
    __shared__ __attribute__((aligned(16))) float Bs[SC_T * SC_LDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l16 = lane & 15, lq = lane >> 4;
    const int a0 = blockIdx.x * SC_T, g = blockIdx.y;
    const int kb_hi = min(nkb, (g + 1) * per);
    const float tau = hyper[1];
    int yi[4];
    float M[4], sum[4], pos[4], cnt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { yi[r] = ylab[a0 + 16 * wv + 4 * lq + r]; M[r] = -INFINITY; sum[r] = pos[r] = cnt[r] = 0.f; }
    for (int kb = g * per; kb < kb_hi; ++kb) {
        const int k0 = kb * SC_T;
        f32x4 acc[4];
        sc_s_tile(Z, Dp, a0, k0, As, Bs, acc);
        int ya[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ya[j] = ylab[k0 + 16 * j + l16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = a0 + 16 * wv + 4 * lq + r;
            float sv[4];
            bool ok[4];
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ok[j] = yi[r] >= 0 && ya[j] >= 0 && (k0 + 16 * j + l16) != i;
                sv[j] = acc[j][r] / tau;
                if (ok[j]) m = fmaxf(m, sv[j]);
            }
            const float Mn = fmaxf(M[r], sc_row_max(m));
            float ts = 0.f, tp = 0.f, tc = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ts += ok[j] ? expf(sv[j] - Mn) : 0.f;
                const bool p = ok[j] && ya[j] == yi[r];
                tp += p ? sv[j] : 0.f;
                tc += p ? 1.f : 0.f;
            }
            sum[r] = (M[r] > -INFINITY ? sum[r] * expf(M[r] - Mn) : 0.f) + sc_row_sum(ts);
            pos[r] += sc_row_sum(tp);
            cnt[r] += sc_row_sum(tc);
            M[r] = Mn;
        }
    }
    if (l16 == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<f32x4*>(part + ((size_t)g * Np + a0 + 16 * wv + 4 * lq + r) * 4) = f32x4{M[r], sum[r], pos[r], cnt[r]};
    }
}

// One lane per row of the padded range.  row_terms[i] = (lse, n, l, w l); rows outside V: zeros, rows of V without a positive: l = 0.
__global__ __launch_bounds__(256) void m2f_supcon_rows_kernel(const float* __restrict__ part, int nkb, int Np, int N,
                                                              const int* __restrict__ ylab, const float* __restrict__ class_w,
                                                              const float* __restrict__ hyper, float* __restrict__ lse,
                                                              float* __restrict__ ninv, float* __restrict__ coef,
                                                              float* __restrict__ row_terms, float* __restrict__ loss_terms) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Np) return;
    const float lambda = hyper[0];
    const int y = ylab[i];
    float M = -INFINITY;
    for (int kb = 0; kb < nkb; ++kb) M = fmaxf(M, part[((size_t)kb * Np + i) * 4]);
    float sum = 0.f, pos = 0.f, cnt = 0.f;
    for (int kb = 0; kb < nkb; ++kb) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(part + ((size_t)kb * Np + i) * 4);
        sum += p[0] > -INFINITY ? p[1] * expf(p[0] - M) : 0.f;
        pos += p[2];
        cnt += p[3];
    }
    const bool any = y >= 0 && M > -INFINITY, has = any && cnt > 0.f;
    const float L = any ? M + logf(sum) : 0.f;
    const float l = has ? L - pos / cnt : 0.f;
    const float w = has ? (class_w ? class_w[y] : 1.f) : 0.f;
    lse[i] = L;
    ninv[i] = has ? 1.0f / cnt : 0.f;
    coef[i] = has ? lambda * w : 0.f;
    if (i < N) {
        *reinterpret_cast<f32x4*>(row_terms + (size_t)i * 4) = f32x4{L, has ? cnt : 0.f, l, w * l};
        if (loss_terms && has) loss_terms[2 * i] = loss_terms[2 * i] + lambda * (w * l);
    }
}

// Workgroup (anchor block, key group g): the group's pairs of key blocks g * ppg .. in order.  Per pair: S and the coefficient tile G of
// each key block into LDS, then dz[64 rows][SC_NC columns at a time] += G Z_k over the pair - the accumulators start from what the
// previous pair of THIS workgroup left in dzp[g] (the same lane wrote it), so a group's partial has one order whatever its length.
__global__ __launch_bounds__(256) void m2f_supcon_bwd_kernel(const float* __restrict__ Z, const int* __restrict__ ylab,
                                                             const float* __restrict__ hyper, const float* __restrict__ lse,
                                                             const float* __restrict__ ninv, const float* __restrict__ coef,
                                                             int Np, int Dp, int nkb, int ppg, float* __restrict__ dzp) {
    constexpr int STAGE = SC_T * SC_LDZ > 2 * SC_T * SC_LDS ? SC_T * SC_LDZ : 2 * SC_T * SC_LDS;
    __shared__ __attribute__((aligned(16))) float stage[STAGE];            // the S product's two slabs, then the key slab of G Z
    __shared__ __attribute__((aligned(16))) float Gs[SC_KG * SC_T * SC_LDG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l16 = lane & 15, lq = lane >> 4;
    const int a0 = blockIdx.x * SC_T, g = blockIdx.y;
    const int npairs = (nkb + SC_KG - 1) / SC_KG, p_lo = g * ppg, p_hi = min(npairs, p_lo + ppg);
    const float tau = hyper[1];
    int yi[4];
    float ci[4], li[4], ni[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = a0 + 16 * wv + 4 * lq + r;
        yi[r] = ylab[i]; ci[r] = coef[i]; li[r] = lse[i]; ni[r] = ninv[i];
    }
    const int sr = tid >> 4, sc = (tid & 15) * 4;          // phase 2: this thread stages rows sr, sr + 16, sr + 32, sr + 48, columns sc .. sc + 3
    float* const out = dzp + ((size_t)g * Np + a0 + 16 * wv + 4 * lq) * Dp + l16;
    for (int pr = p_lo; pr < p_hi; ++pr) {
        const int kcount = min(SC_KG, nkb - pr * SC_KG);
        for (int kbl = 0; kbl < kcount; ++kbl) {
            const int k0 = (pr * SC_KG + kbl) * SC_T;
            f32x4 acc[4];
            sc_s_tile(Z, Dp, a0, k0, stage, stage + SC_T * SC_LDS, acc);
            float* Gt = Gs + kbl * SC_T * SC_LDG;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = k0 + 16 * j + l16;
                const int ya = ylab[a];
                const float ca = coef[a], la = lse[a], na = ninv[a];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = a0 + 16 * wv + 4 * lq + r;
                    const bool ok = yi[r] >= 0 && ya >= 0 && a != i, same = yi[r] == ya;
                    const float s = acc[j][r] / tau;
                    // (a row without a positive has c = 0 and may have no lse worth the name: its term is SELECTED away, never multiplied)
                    const float t1 = ci[r] != 0.f ? ci[r] * (expf(s - li[r]) - (same ? ni[r] : 0.f)) : 0.f;
                    const float t2 = ca != 0.f ? ca * (expf(s - la) - (same ? na : 0.f)) : 0.f;
                    Gt[(16 * wv + 4 * lq + r) * SC_LDG + 16 * j + l16] = ok ? t1 + t2 : 0.f;
                }
            }
        }
        // the key slab one step ahead in registers; step st = (column chunk st / kcount, key block st % kcount)
        const int steps = (Dp / SC_NC) * kcount;
        auto slab = [&](int st) { return Z + (size_t)((pr * SC_KG + st % kcount) * SC_T + sr) * Dp + (st / kcount) * SC_NC + sc; };
        f32x4 rz[4];
        {
            const float* p = slab(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) rz[q] = *reinterpret_cast<const f32x4*>(p + (size_t)16 * q * Dp);
        }
        f32x4 acc2[4];
        for (int st = 0; st < steps; ++st) {
            const int kbl = st % kcount, c0 = (st / kcount) * SC_NC;
            __syncthreads();                                // (the S slabs / the previous key slab are read; the first time: Gs is written)
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(stage + (sr + 16 * q) * SC_LDZ + sc) = rz[q];
            __syncthreads();
            if (st + 1 < steps) {
                const float* p = slab(st + 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) rz[q] = *reinterpret_cast<const f32x4*>(p + (size_t)16 * q * Dp);
            }
            if (kbl == 0) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc2[n][r] = pr > p_lo ? out[(size_t)r * Dp + c0 + 16 * n] : 0.f;
            }
            const float* gr = Gs + kbl * SC_T * SC_LDG + (16 * wv + l16) * SC_LDG + lq;
            const float* zr = stage + lq * SC_LDZ + l16;
#pragma unroll
            for (int k4 = 0; k4 < SC_T; k4 += 4) {
                const float a = gr[k4];
#pragma unroll
                for (int n = 0; n < 4; ++n) acc2[n] = sc_mfma(a, zr[k4 * SC_LDZ + 16 * n], acc2[n]);
            }
            if (kbl == kcount - 1) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[(size_t)r * Dp + c0 + 16 * n] = acc2[n][r];
            }
        }
    }
}

// One wave per row i < N: dz = the groups' partials in group order; dfeat = ((dz - (dz . z) z) / ||h||) / tau, zeros outside V.
__global__ __launch_bounds__(256) void m2f_supcon_dfeat_kernel(const float* __restrict__ dzp, int G, int Np, int Dp,
                                                               const float* __restrict__ Z, const float* __restrict__ rinv,
                                                               const float* __restrict__ hyper, int N, int D,
                                                               float* __restrict__ dfeat, int ldd) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                     // (wave-uniform)
    const float tau = hyper[1], ri = rinv[i];
    auto dz = [&](int c) {
        float v = 0.f;
        for (int g = 0; g < G; ++g) v += dzp[((size_t)g * Np + i) * Dp + c];
        return v;
    };
    float dot = 0.f;
    for (int c = lane; c < D; c += 64) dot += dz(c) * Z[(size_t)i * Dp + c];
    dot = m2f_wave_sum(dot);
    for (int c = lane; c < D; c += 64)
        dfeat[(size_t)i * ldd + c] = ri > 0.f ? ((dz(c) - dot * Z[(size_t)i * Dp + c]) * ri) / tau : 0.f;
}

// loss_out[3] = (ACC: +=) sum of w l over the rows, in the finalize launch's order; scale[0] = what that launch multiplies dlogits by
// (1 / den from the same block sum of the same terms, or 1 without normalise; den == 0: 0, nothing to scale)
template <bool ACC>
__global__ __launch_bounds__(256) void m2f_supcon_tail_kernel(const float* __restrict__ row_terms, const float* __restrict__ loss_terms,
                                                              int T, float* __restrict__ loss_out, float* __restrict__ scale, int normalise) {
    float r4[4], s[2];
    m2f_block_sum_terms<4>(row_terms, T, r4);
    m2f_block_sum_terms<2>(loss_terms, T, s);
    if (threadIdx.x == 0) {
        if constexpr (ACC) loss_out[3] = loss_out[3] + r4[3];
        else loss_out[3] = r4[3];
        scale[0] = normalise ? (s[1] > 0.f ? 1.0f / s[1] : 0.f) : 1.f;
    }
}

// dh[i, :] += (h[i, :] > 0 ? gate_scale : 0) * scale * dfeat[i, :], the bf16 shadow of dh rewritten when it has one
__global__ __launch_bounds__(256) void m2f_supcon_add_kernel(float* __restrict__ dh, const float* __restrict__ h,
                                                             const float* __restrict__ dfeat, const float* __restrict__ scale, int T, int d,
                                                             int ld, float gate_scale, int write16, ShadowMap sh) {
    const float sc = scale[0];
    uint16_t* dh16 = write16 ? m2f_shadow_of(sh, dh) : nullptr;
    const size_t n = (size_t)T * d;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / d), c = (int)(e - (size_t)r * d);
        const size_t o = (size_t)r * ld + c;
        const float v = dh[o] + (h[o] > 0.f ? gate_scale : 0.f) * (sc * dfeat[o]);
        dh[o] = v;
        if (dh16) dh16[o] = m2f_bf16_bits(v);
    }
}

inline int sc_up(int x) { return (x + SC_T - 1) / SC_T * SC_T; }

// The grids, from N alone.  Forward: the nkb key blocks in at most SC_GF groups of `per`; backward: the pairs of key blocks in at most
// SC_GB groups of `ppg` (both bound the workspace: the partials are per group).
constexpr int SC_GF = 16, SC_GB = 8;
struct ScGrid { int Np, Dp, nkb, per, GF, ppg, G; };
inline ScGrid sc_grid(int N, int D) {
    ScGrid q;
    q.Np = sc_up(N); q.Dp = sc_up(D); q.nkb = q.Np / SC_T;
    q.per = m2f_cdiv(q.nkb, std::min(q.nkb, SC_GF)); q.GF = m2f_cdiv(q.nkb, q.per);
    const int npairs = m2f_cdiv(q.nkb, SC_KG);
    q.ppg = m2f_cdiv(npairs, std::min(npairs, SC_GB)); q.G = m2f_cdiv(npairs, q.ppg);
    return q;
}

}  // namespace

// Z [Np, Dp] | dzp [G, Np, Dp] | part [GF, Np, 4] | rinv, lse, ninv, coef [Np] each | ylab int32 [Np]
size_t m2f_supcon_ws_floats(int N, int D) {
    if (N < 1 || D < 1) return 0;
    const ScGrid q = sc_grid(N, D);
    return (size_t)q.Np * q.Dp * (1 + q.G) + (size_t)q.GF * q.Np * 4 + (size_t)5 * q.Np;
}

hipError_t m2f_launch_supcon(const SupconArgs& a, hipStream_t stream) {
    if (!a.feat || !a.labels || !a.hyper || !a.ws || !a.row_terms || !a.dfeat || a.N < 1 || a.D < 1 || a.ld < a.D || a.ldd < a.D ||
        a.C < 1 || (reinterpret_cast<uintptr_t>(a.ws) & 15) || (reinterpret_cast<uintptr_t>(a.row_terms) & 15))
        return hipErrorInvalidValue;
    const ScGrid q = sc_grid(a.N, a.D);
    const int Np = q.Np, Dp = q.Dp;
    float* Z = a.ws;
    float* dzp = Z + (size_t)Np * Dp;
    float* part = dzp + (size_t)q.G * Np * Dp;
    float* rinv = part + (size_t)q.GF * Np * 4;
    float* lse = rinv + Np;
    float* ninv = lse + Np;
    float* coef = ninv + Np;
    int* ylab = reinterpret_cast<int*>(coef + Np);
    hipLaunchKernelGGL(m2f_supcon_prep_kernel, dim3(Np / 4), dim3(256), 0, stream, a.feat, a.N, a.D, a.ld, a.labels, a.C, Dp, Z, rinv, ylab);
    hipLaunchKernelGGL(m2f_supcon_fwd_kernel, dim3(q.nkb, q.GF), dim3(256), 0, stream, Z, ylab, a.hyper, Np, Dp, q.nkb, q.per, part);
    hipLaunchKernelGGL(m2f_supcon_rows_kernel, dim3(m2f_cdiv(Np, 256)), dim3(256), 0, stream, part, q.GF, Np, a.N, ylab, a.class_w, a.hyper,
                       lse, ninv, coef, a.row_terms, a.loss_terms);
    hipLaunchKernelGGL(m2f_supcon_bwd_kernel, dim3(q.nkb, q.G), dim3(256), 0, stream, Z, ylab, a.hyper, lse, ninv, coef, Np, Dp, q.nkb, q.ppg, dzp);
    hipLaunchKernelGGL(m2f_supcon_dfeat_kernel, dim3(m2f_cdiv(a.N, 4)), dim3(256), 0, stream, dzp, q.G, Np, Dp, Z, rinv, a.hyper, a.N, a.D,
                       a.dfeat, a.ldd);
    return hipGetLastError();
}

hipError_t m2f_launch_supcon_tail(const float* row_terms, const float* loss_terms, int T, float* loss_out, float* scale, int normalise,
                                  hipStream_t stream, int accumulate) {
    if (!row_terms || !loss_terms || !loss_out || !scale || T < 1) return hipErrorInvalidValue;
    if (accumulate) hipLaunchKernelGGL(m2f_supcon_tail_kernel<true>, dim3(1), dim3(256), 0, stream, row_terms, loss_terms, T, loss_out, scale, normalise);
    else hipLaunchKernelGGL(m2f_supcon_tail_kernel<false>, dim3(1), dim3(256), 0, stream, row_terms, loss_terms, T, loss_out, scale, normalise);
    return hipGetLastError();
}

hipError_t m2f_launch_supcon_add(float* dh, const float* h, const float* dfeat, const float* scale, int T, int d, int ld, float gate_scale,
                                 int write16, ShadowMap sh, hipStream_t stream) {
    if (!dh || !h || !dfeat || !scale || T < 1 || d < 1 || ld < d) return hipErrorInvalidValue;
    const size_t n = (size_t)T * d;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(m2f_supcon_add_kernel, dim3(blocks), dim3(256), 0, stream, dh, h, dfeat, scale, T, d, ld, gate_scale, write16, sh);
    return hipGetLastError();
}
