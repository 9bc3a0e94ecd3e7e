// Linear-chain CRF over a dialogue's labels (CrfArgs / CrfViterbiArgs / CrfFilterArgs, ops.h): negative log likelihood with its
// gradients, the Viterbi path, and the forward filter of the streaming path.
//
// One 16-lane row of a wave owns one dialogue (one stream slot): lane j owns class j, holds column transitions[:, j] (and, for the
// backward sweep, row transitions[j, :]) in registers, and exchanges the 16 per-class values of a step with cross-lane reads inside the
// row - no LDS, no barrier.  A workgroup is ONE wave = four dialogues, so that a batch spreads over the CUs: the recursion is a chain of
// dependent steps, latency is all there is.  Every loop runs to the wave's longest dialogue with the shorter ones predicated off, so the
// cross-lane reads are never executed under divergent control flow.
//
// Arithmetic.  alpha is carried NORMALISED in log space: phi_k = a_k - logsumexp(a_k), the step's logsumexp added to the dialogue's
// numerator on its own (minus the step's share of score(y), so that the running sum stays small).  beta is carried relative to its max.
// Marginals are softmax(phi_k + psi_k) - formed from the relative values, never from a difference of two large log-sums - and the pair
// marginal is P(y_k = j) * P(y_{k-1} = i | y_k = j, e_1..k-1) = P_k(j) * softmax_i(phi_{k-1}(i) + transitions[i, j]).
// Every logsumexp subtracts its max first: transitions of -1e4 and logit margins of +-120 stay finite.
// crf_forward_step is the ONE step function of the loss and the filter: the filter's phi has the loss kernel's bits.
#include "common.h"
#include "ops.h"

namespace {

__device__ __forceinline__ float crf_row_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 16));
    return v;
}
__device__ __forceinline__ float crf_row_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    return v;
}
// logsumexp over the 16-lane row; lanes that own no class hand in -inf (at least one lane is finite)
__device__ __forceinline__ float crf_row_lse(float v) {
    const float m = crf_row_max(v);
    return m + logf(crf_row_sum(expf(v - m)));
}

// a[j] of one chain row: start[j] + e[j] on a dialogue's first row, e[j] + logsumexp_i(phi[i] + transitions[i, j]) after it; -inf on a
// lane without a class.  col[i] = transitions[i, j].
__device__ __forceinline__ float crf_forward_step(float phi, float e, const float (&col)[16], float start, bool first, int C, bool own) {
    float u[16];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        u[i] = __shfl(phi, i, 16) + col[i];
        if (i < C) mx = fmaxf(mx, u[i]);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += (i < C) ? expf(u[i] - mx) : 0.f;
    const float a = first ? start + e : e + (mx + logf(s));
    return own ? a : -INFINITY;
}

struct CrfSpan { int r0, len; };
// rows of dialogue b: cu[b] .. cu[b+1]-1 (packed and long-dialogue plans) or b*L .. b*L+L-1 (padded plans); clipped to [0, T)
__device__ __forceinline__ CrfSpan crf_span(const int32_t* __restrict__ cu, int B, int L, int T, int b) {
    CrfSpan s = {0, 0};
    if (b >= B) return s;
    int r0 = cu ? cu[b] : b * L, r1 = cu ? cu[b + 1] : b * L + L;
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > T ? T : r1;
    s.r0 = r0;
    s.len = r1 > r0 ? r1 - r0 : 0;
    return s;
}
// the rows behind the last dialogue (a packed plan larger than its batch): the last dialogue's lanes clear them
__device__ __forceinline__ int crf_tail_begin(const int32_t* __restrict__ cu, int B, int L, int T) {
    const int e = cu ? cu[B] : B * L;
    return e < 0 ? 0 : (e > T ? T : e);
}
__device__ __forceinline__ int crf_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// Saved row of the backward sweep, at the dialogue's k-th CHAIN position (row r0 + k of ws, compacted: the sweep's addresses do not depend
// on what it loads): [phi (C) | e (C) | label | token row], 2C + 2 floats.
// MODE 0: the loss terms only (no gradient, ws untouched); 1: and dlogits; 2: and the parameter gradient's partials
template <int MODE>
__global__ __launch_bounds__(64) void m2f_crf_nll_kernel(const CrfArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int b = blockIdx.x * 4 + (lane >> 4);
    const int C = a.C, W = 2 * C + 2, P = C * C + 2 * C;
    constexpr bool PGRAD = MODE == 2;
    const bool own = j < C;
    const CrfSpan sp = crf_span(a.cu_seqlens, a.B, a.L, a.T, b);
    float col[16], row[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        col[i] = (own && i < C) ? a.params[i * C + j] : 0.f;
        row[i] = (own && i < C) ? a.params[j * C + i] : 0.f;
    }
    const float start = own ? a.params[C * C + j] : 0.f, end = own ? a.params[C * C + C + j] : 0.f;
    const int maxlen = crf_wave_max(sp.len);

    // ---- forward sweep: labels two rows ahead, logits (of labelled rows only) one row ahead ----
    float phi = 0.f, num = 0.f;
    int n = 0, yprev = 0, first_row = -1;
    int64_t y1 = sp.len > 0 ? a.labels[sp.r0] : -1, y2 = sp.len > 1 ? a.labels[sp.r0 + 1] : -1;
    bool v1 = y1 >= 0 && y1 < C;
    float e1 = (v1 && own) ? a.logits[(size_t)sp.r0 * C + j] : 0.f;
    for (int k = 0; k < maxlen; ++k) {
        const bool in = k < sp.len;
        const int r = sp.r0 + k;
        const bool valid = in && v1;
        const int y = valid ? (int)y1 : 0;
        const float e = e1;
        y1 = y2;
        y2 = (k + 2 < sp.len) ? a.labels[r + 2] : -1;
        v1 = y1 >= 0 && y1 < C;
        e1 = (k + 1 < sp.len && v1 && own) ? a.logits[(size_t)(r + 1) * C + j] : 0.f;

        const bool first = n == 0;
        const float av = crf_forward_step(phi, e, col, start, first, C, own);
        const float l = crf_row_lse(av);
        float tsel = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) tsel = (i == yprev) ? col[i] : tsel;
        const float sc = __shfl(e, y, 16) + (first ? __shfl(start, y, 16) : __shfl(tsel, y, 16));
        if (valid) {
            phi = av - l;
            num += l - sc;
            if constexpr (MODE > 0) {
                float* w = a.ws + (size_t)(sp.r0 + n) * W;
                if (own) { w[j] = phi; w[C + j] = e; }
                w[2 * C] = __int_as_float(y); w[2 * C + 1] = __int_as_float(r);     // every lane of the row: each reads back its own store
            }
            if (first) first_row = r;
            yprev = y;
            ++n;
        }
        if (in) {
            if (j == 0) { a.loss_terms[2 * r] = 0.f; a.loss_terms[2 * r + 1] = valid ? 1.f : 0.f; }
            if (MODE > 0 && !valid && own) a.dlogits[(size_t)r * C + j] = 0.f;
        }
    }
    {   // the end term closes the numerator; it lands on the dialogue's first chain row
        const float l = crf_row_lse(own ? phi + end : -INFINITY);
        const float sc = __shfl(end, yprev, 16);
        if (n > 0 && j == 0) a.loss_terms[2 * first_row] = num + (l - sc);
    }
    if (b == a.B - 1)
        for (int r = crf_tail_begin(a.cu_seqlens, a.B, a.L, a.T) + j; r < a.T; r += 16) {
            a.loss_terms[2 * r] = 0.f; a.loss_terms[2 * r + 1] = 0.f;
            if constexpr (MODE > 0)
                for (int c = 0; c < C; ++c) a.dlogits[(size_t)r * C + c] = 0.f;
        }
    if constexpr (MODE == 0) return;

    // ---- backward sweep over the saved chain rows, last to first; the row below is loaded one step ahead ----
    // (a lane reads back only what it stored itself)
    float dT[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dT[i] = 0.f;
    float dstart = 0.f, dend = 0.f;
    float psi = own ? end : 0.f;
    const int maxn = crf_wave_max(n);
    const float* wb = a.ws + (size_t)sp.r0 * W;
    float phi_c = 0.f, e_c = 0.f; int y_c = 0, r_c = 0;
    float phi_p = 0.f, e_p = 0.f; int y_p = 0, r_p = 0;
    if (n > 0) {
        const float* w = wb + (size_t)(n - 1) * W;
        phi_p = own ? w[j] : 0.f; e_p = own ? w[C + j] : 0.f; y_p = __float_as_int(w[2 * C]); r_p = __float_as_int(w[2 * C + 1]);
    }
    for (int kk = maxn - 1; kk >= 0; --kk) {
        const bool on = kk < n;
        if (on) { phi_c = phi_p; e_c = e_p; y_c = y_p; r_c = r_p; }
        if (on && kk > 0) {
            const float* w = wb + (size_t)(kk - 1) * W;
            phi_p = own ? w[j] : 0.f; e_p = own ? w[C + j] : 0.f; y_p = __float_as_int(w[2 * C]); r_p = __float_as_int(w[2 * C + 1]);
        }
        // marginal of the row from the relative values
        const float q = own ? phi_c + psi : -INFINITY;
        const float ex = expf(q - crf_row_max(q));
        const float p = ex / crf_row_sum(ex);
        const float g = p - ((j == y_c) ? 1.f : 0.f);
        if (on && own) a.dlogits[(size_t)r_c * C + j] = g;
        if constexpr (PGRAD) {
            if (on && kk == n - 1) dend = g;
            if (on && kk == 0) dstart = g;
            // pair marginal with the chain row below: column j of it on lane j
            float u[16];
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                u[i] = __shfl(phi_p, i, 16) + col[i];
                if (i < C) mx = fmaxf(mx, u[i]);
            }
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { u[i] = (i < C) ? expf(u[i] - mx) : 0.f; s += u[i]; }
            const float scale = p / s;
            if (on && kk > 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) dT[i] += u[i] * scale - ((i == y_p && j == y_c) ? 1.f : 0.f);
            }
        }
        // psi of the row below, on lane i: logsumexp_j(transitions[i, j] + e[j] + psi[j]), carried relative to its max
        const float wv = own ? e_c + psi : 0.f;
        float v[16];
        float mx2 = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = __shfl(wv, i, 16) + row[i];
            if (i < C) mx2 = fmaxf(mx2, v[i]);
        }
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s2 += (i < C) ? expf(v[i] - mx2) : 0.f;
        const float pn = mx2 + logf(s2);
        const float pm = crf_row_max(own ? pn : -INFINITY);
        if (on) psi = own ? pn - pm : 0.f;
    }
    if constexpr (PGRAD) {
        if (b < a.B && own) {
            float* part = a.partial + (size_t)b * P;      // a dialogue without a chain row writes its zeros
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i < C) part[i * C + j] = dT[i];
            part[C * C + j] = dstart;
            part[C * C + C + j] = dend;
        }
    }
}

// Parameter gradient: the dialogues' partials added in dialogue order by one thread per element - a fixed order, no atomics.
// normalise: divided by the den that m2f_loss_finalize_kernel wrote (loss_out[1]) in front of this launch, as it scales dlogits.
__global__ __launch_bounds__(64) void m2f_crf_grad_reduce_kernel(const float* __restrict__ partial, int B, int P,
                                                                 const float* __restrict__ loss_out, int normalise,
                                                                 float* __restrict__ grad) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += partial[(size_t)b * P + p];
    if (normalise && loss_out[1] != 0.f) s *= 1.0f / loss_out[1];      // (no labelled row at all: every partial is an exact zero and stays one)
    grad[p] = s;
}

// Viterbi.  delta is carried relative to its max, the maxima added to the path score on their own.  First-max rule: the lowest class
// wins a tie, in the recursion (ascending i, strict >) and at the end (the row argmax prefers the lower lane).
// Saved row at the k-th chain position (row r0 + k of ws, 5 ints): 16 backpointer bytes (byte j = lane j's) | token row.
__global__ __launch_bounds__(64) void m2f_crf_viterbi_kernel(const CrfViterbiArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int b = blockIdx.x * 4 + (lane >> 4);
    const int C = a.C;
    const bool own = j < C;
    const CrfSpan sp = crf_span(a.cu_seqlens, a.B, a.L, a.T, b);
    float col[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) col[i] = (own && i < C) ? a.params[i * C + j] : 0.f;
    const float start = own ? a.params[C * C + j] : 0.f, end = own ? a.params[C * C + C + j] : 0.f;
    const int maxlen = crf_wave_max(sp.len);

    float delta = 0.f, score = 0.f;
    int n = 0;
    uint8_t m1 = sp.len > 0 ? (a.mask ? a.mask[sp.r0] : 0) : 1, m2 = sp.len > 1 ? (a.mask ? a.mask[sp.r0 + 1] : 0) : 1;
    float e1 = (!m1 && own) ? a.logits[(size_t)sp.r0 * C + j] : 0.f;
    for (int k = 0; k < maxlen; ++k) {
        const bool in = k < sp.len;
        const int r = sp.r0 + k;
        const bool valid = in && !m1;
        const float e = e1;
        m1 = m2;
        m2 = (k + 2 < sp.len) ? (a.mask ? a.mask[r + 2] : 0) : 1;
        e1 = (k + 1 < sp.len && !m1 && own) ? a.logits[(size_t)(r + 1) * C + j] : 0.f;

        float best = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float u = __shfl(delta, i, 16) + col[i];
            if (i < C && u > best) { best = u; arg = i; }
        }
        const bool first = n == 0;
        const float d = own ? (first ? start + e : best + e) : -INFINITY;
        const float m = crf_row_max(d);
        if (valid) {
            delta = d - m;
            score += m;
            int* w = a.ws + (size_t)(sp.r0 + n) * 5;
            reinterpret_cast<uint8_t*>(w)[j] = (uint8_t)(first ? 0 : arg);
            w[4] = r;                                       // every lane of the row: each reads back its own store
            ++n;
        }
        if (in && !valid && j == 0) a.pred[r] = -1;
    }
    if (b == a.B - 1)
        for (int r = crf_tail_begin(a.cu_seqlens, a.B, a.L, a.T) + j; r < a.T; r += 16) a.pred[r] = -1;

    // the end of the path: first max of delta + end over the row
    float fv = own ? delta + end : -INFINITY;
    int cur = j;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const float ov = __shfl_xor(fv, o, 16);
        const int oc = __shfl_xor(cur, o, 16);
        if (ov > fv || (ov == fv && oc < cur)) { fv = ov; cur = oc; }
    }
    if (b < a.B && j == 0) a.score[b] = n > 0 ? score + fv : 0.f;

    // ---- back trace: the saved row below is loaded one step ahead; the pointer is picked from the row's lanes ----
    const int maxn = crf_wave_max(n);
    const int* wb = a.ws + (size_t)sp.r0 * 5;
    int bp_p = 0, r_p = 0, bp_c = 0, r_c = 0;
    if (n > 0) { const int* w = wb + (size_t)(n - 1) * 5; bp_p = reinterpret_cast<const uint8_t*>(w)[j]; r_p = w[4]; }
    for (int kk = maxn - 1; kk >= 0; --kk) {
        const bool on = kk < n;
        if (on) { bp_c = bp_p; r_c = r_p; }
        if (on && kk > 0) { const int* w = wb + (size_t)(kk - 1) * 5; bp_p = reinterpret_cast<const uint8_t*>(w)[j]; r_p = w[4]; }
        const int prev = __shfl(bp_c, cur, 16);
        if (on) {
            if (j == 0) a.pred[r_c] = cur;
            cur = prev;
        }
    }
}

// Forward filter of the streams: slot s takes rows s*rows .. s*rows + n_new[s] - 1 of the logits in order (n_new null: one row per
// active slot); phi[s] = log P(label of the slot's last utterance | its dialogue so far), the END term not applied.
// count[s] (the utterances the slot holds BEFORE this launch) is read, never written: the launch behind this one advances it.
__global__ __launch_bounds__(64) void m2f_crf_filter_kernel(const CrfFilterArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int s = blockIdx.x * 4 + (lane >> 4);
    const int C = a.C;
    const bool own = j < C;
    float col[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) col[i] = (own && i < C) ? a.params[i * C + j] : 0.f;
    const float start = own ? a.params[C * C + j] : 0.f;
    int nn = 0, cnt = 0;
    if (s < a.S) {
        const bool act = a.active ? a.active[s] != 0 : true;
        nn = act ? (a.n_new ? a.n_new[s] : 1) : 0;
        nn = nn < 0 ? 0 : (nn > a.rows ? a.rows : nn);
        cnt = a.count[s];
    }
    float phi = (s < a.S && own) ? a.phi[(size_t)s * C + j] : 0.f;
    const int maxn = crf_wave_max(nn);
    float e1 = (nn > 0 && own) ? a.logits[(size_t)s * a.rows * C + j] : 0.f;
    for (int k = 0; k < maxn; ++k) {
        const float e = e1;
        e1 = (k + 1 < nn && own) ? a.logits[((size_t)s * a.rows + k + 1) * C + j] : 0.f;
        const float av = crf_forward_step(phi, e, col, start, cnt + k == 0, C, own);
        const float l = crf_row_lse(av);
        if (k < nn) phi = av - l;
    }
    if (nn > 0 && own) a.phi[(size_t)s * C + j] = phi;
}

}  // namespace

hipError_t m2f_launch_crf_nll(const CrfArgs& a, hipStream_t stream) {
    const dim3 grid(m2f_cdiv(a.B, 4)), block(64);
    if (!a.dlogits && a.partial) return hipErrorInvalidValue;
    if (a.partial) hipLaunchKernelGGL(m2f_crf_nll_kernel<2>, grid, block, 0, stream, a);
    else if (a.dlogits) hipLaunchKernelGGL(m2f_crf_nll_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(m2f_crf_nll_kernel<0>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t m2f_launch_crf_grad_reduce(const float* partial, int B, int C, const float* loss_out, int normalise, float* grad,
                                      hipStream_t stream) {
    const int P = C * C + 2 * C;
    hipLaunchKernelGGL(m2f_crf_grad_reduce_kernel, dim3(m2f_cdiv(P, 64)), dim3(64), 0, stream, partial, B, P, loss_out, normalise, grad);
    return hipGetLastError();
}

hipError_t m2f_launch_crf_viterbi(const CrfViterbiArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_crf_viterbi_kernel, dim3(m2f_cdiv(a.B, 4)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t m2f_launch_crf_filter(const CrfFilterArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(m2f_crf_filter_kernel, dim3(m2f_cdiv(a.S, 4)), dim3(64), 0, stream, a);
    return hipGetLastError();
}
