// The criterion row, written ONCE: the label-smoothed cross entropy of one token row (C <= 16 classes, everything in registers, the
// sixteen classes fully unrolled) and the parts the distillation, focal and R-Drop criteria add to it.  Every kernel that scores a row
// is a thin body over these helpers - rowops.hip: m2f_ce_kernel, m2f_ce_distill_kernel, m2f_ce_focal_kernel<TEACHER>,
// m2f_ce_rdrop_kernel; metrics.hip: m2f_eval_rows_kernel<FOCAL> - so the equalities the suite promises (alpha = 0 and gamma = 0 give the
// plain kernel's bits, the eval loss is the train loss's bits) hold because the statements ARE the same, not because copies were kept
// in step.  tests/golden/criterion_kernel_bits.npz holds the bits from before the copies became this header.
//
// The bits must not depend on who includes the header: every helper turns fp contraction off ITSELF (the pragma at the start of its
// body; the setting travels with the inlined instructions), no sum here may be re-associated, eps * sm / (float)C stays a division, and
// every `valid ? ... : 0.f` stays a select.  A kernel that does not use a field (the eval form never reads W) pays nothing: the
// helpers are inlined and the dead sum is removed.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"

struct CeRow {
    float z[16], w[16];                  // logits (-inf behind C) and class weights (1 without class_w, 0 behind C)
    float m, se, lse;                    // max, sum of expf(z - m), m + logf(se)
    float W, sm;                         // sum of w, -sum of w_c * logp_c
    float wy, logpy;                     // the label's weight and log-probability (0 on an invalid row)
    float eps, num;                      // label_smoothing; the numerator (1 - eps) * -logp_y * w_y + eps * sm / C, 0 on an invalid row
    int64_t y; bool valid;               // valid: 0 <= y < C
    int C;
};

// Forward of row t: load, max, sum of exponentials, lse, W, sm, w_y, logp_y and the numerator.
__device__ __forceinline__ void m2f_ce_row_forward(CeRow& r, const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                   const float* __restrict__ class_w, float label_smoothing, int t, int C) {
#pragma clang fp contract(off)
    r.C = C;
    r.m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        r.z[c] = (c < C) ? logits[(size_t)t * C + c] : -INFINITY;
        r.w[c] = (c < C) ? (class_w ? class_w[c] : 1.f) : 0.f;
        r.m = fmaxf(r.m, r.z[c]);
    }
    r.se = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) r.se += (c < C) ? expf(r.z[c] - r.m) : 0.f;
    r.lse = r.m + logf(r.se);
    r.y = labels[t];
    r.valid = (r.y >= 0) && (r.y < C);
    r.wy = 0.f; r.logpy = 0.f; r.W = 0.f; r.sm = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < C) {
            const float lp = r.z[c] - r.lse;
            r.W += r.w[c];
            r.sm -= r.w[c] * lp;
            if (r.valid && c == (int)r.y) { r.wy = r.w[c]; r.logpy = lp; }
        }
    }
    r.eps = label_smoothing;
    r.num = r.valid ? ((1.f - r.eps) * (-r.logpy) * r.wy + r.eps * r.sm / (float)r.C) : 0.f;
}

// Probability of class c as the gradient uses it
__device__ __forceinline__ float m2f_ce_row_p(const CeRow& r, int c) {
#pragma clang fp contract(off)
    return expf(r.z[c] - r.lse);
}

// UNNORMALISED gradient of the numerator with respect to z_c (c < C), p = m2f_ce_row_p(r, c); 0 on an invalid row
__device__ __forceinline__ float m2f_ce_row_grad(const CeRow& r, int c, float p) {
#pragma clang fp contract(off)
    float g = 0.f;
    if (r.valid) g = (1.f - r.eps) * r.wy * (p - ((c == (int)r.y) ? 1.f : 0.f)) + (r.eps / (float)r.C) * (r.W * p - r.w[c]);
    return g;
}

// ---- focal part: the hard-label term scaled by omp^gamma ----------------------------------------------------------------------
//   omp is the other classes' probabilities ADDED (c != y), not 1 - p_y: at a margin of 20 p_y rounds to 1 and 1 - p_y to 0 or to one
//   ulp of 1, while the sum keeps its own 24 bits.  For the same reason the y column's slope is -omp, not p_y - 1.
//   The slope term ce * gamma * omp^(gamma-1) * p_y * d_c (d_c = p_c, d_y = -omp) is computed as ce * gamma * omp^gamma * p_y * r_c with
//   r_c = p_c / omp <= 1, r_y = -1: no factor exceeds 1, so a gamma in (0, 1) cannot overflow omp^(gamma-1) at a tiny omp.
//   omp == 0 (every other expf underflowed): factor, slope and every r_c are SELECTED to 0 for gamma > 0; logf / powf never see the zero.
//   gamma == 0 SELECTS the unscaled values, so it gives the plain (with a teacher: the distillation) kernel's bits.
struct CeFocal {
    float p[16];                         // m2f_ce_row_p of every class (0 behind C)
    float omp, py, f, num_f, slope;      // f = m2f_focal_factor(omp, gamma); num_f: the scaled numerator
    bool focal, live;                    // gamma > 0; ... and omp > 0
};

__device__ __forceinline__ void m2f_ce_row_focal(CeFocal& k, const CeRow& r, float gamma) {
#pragma clang fp contract(off)
    k.omp = 0.f; k.py = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        k.p[c] = (c < r.C) ? m2f_ce_row_p(r, c) : 0.f;
        if (c < r.C) {
            if (r.valid && c == (int)r.y) k.py = k.p[c];
            else k.omp += k.p[c];
        }
    }
    k.focal = gamma > 0.f;
    k.live = k.focal && k.omp > 0.f;
    k.f = m2f_focal_factor(k.omp, gamma);
    k.slope = k.live ? r.num * gamma * k.f * k.py : 0.f;
    k.num_f = k.focal ? k.f * r.num : r.num;
}

// the focal gradient of class c from the plain one, g = m2f_ce_row_grad(r, c, k.p[c])
__device__ __forceinline__ float m2f_ce_focal_grad(const CeFocal& k, const CeRow& r, int c, float g) {
#pragma clang fp contract(off)
    const float rc = k.live ? ((c == (int)r.y) ? -1.f : k.p[c] / k.omp) : 0.f;
    return k.focal ? (k.f * g + k.slope * rc) : g;
}

// ---- teacher part: q = softmax(z / tau), pt = softmax(u / tau), KL = sum_c pt_c (logpt_c - logq_c) ---------------------------
//   alpha = 0 gives the plain bits: (1 - 0) * x + 0 * finite is exact.  logpt / logq come from the log-softmax (u_c / tau - lse),
//   never from log(p): a teacher probability that underflows contributes 0 * finite = 0.  An invalid row (label -1 or out of range) is
//   a SELECT of zeros in the kernels, whatever its teacher row holds (NaN, inf).
struct CeTeacher {
    float zt[16], u[16];                 // z / tau, teacher / tau (-inf behind C)
    float lsz, lsu;                      // their log-sum-exps
    float oma, kd, gd;                   // 1 - alpha; alpha * tau^2 * w_y (the KL's weight); alpha * tau * w_y (its gradient's)
};

__device__ __forceinline__ void m2f_ce_row_teacher(CeTeacher& k, const CeRow& r, const float* __restrict__ teacher, int t, float alpha,
                                                   float tau) {
#pragma clang fp contract(off)
    const int C = r.C;
    float mz = -INFINITY, mu = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        k.zt[c] = (c < C) ? r.z[c] / tau : -INFINITY;
        k.u[c] = (c < C) ? teacher[(size_t)t * C + c] / tau : -INFINITY;
        mz = fmaxf(mz, k.zt[c]);
        mu = fmaxf(mu, k.u[c]);
    }
    float sz = 0.f, su = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        sz += (c < C) ? expf(k.zt[c] - mz) : 0.f;
        su += (c < C) ? expf(k.u[c] - mu) : 0.f;
    }
    k.lsz = mz + logf(sz); k.lsu = mu + logf(su);
    k.oma = 1.f - alpha;
    k.kd = alpha * tau * tau * r.wy; k.gd = alpha * tau * r.wy;
}

// class c (c < C) of the teacher term: adds pt_c * (logpt_c - logq_c) to kl and returns q_c - pt_c
__device__ __forceinline__ float m2f_ce_teacher_class(const CeTeacher& k, int c, float& kl) {
#pragma clang fp contract(off)
    const float lq = k.zt[c] - k.lsz, lpt = k.u[c] - k.lsu;
    const float q = expf(lq), pt = expf(lpt);
    kl += pt * (lpt - lq);
    return q - pt;
}

// ---- twin part of R-Drop: s = 0.5 * sum_c (p_c - q_c)(logp_c - logq_c) against row tr of the SAME logits buffer ---------------
//   q is computed as the twin computes its own p (expf((u_c - max) - logf(sum))), so s has the same bits on both rows of a pair, and
//   twins with equal logits give s = 0 and a KL gradient of exactly 0.  logp - logq comes from the two log-softmaxes, never from
//   log(p): a probability that underflows contributes 0 * finite = 0.  has == false (no twin): the caller passes tr = the row itself and
//   everything here is SELECTED to the plain term.
struct CeTwin {
    float p[16], q[16], e[16];
    float ebar, ws;                      // sum_c p_c e_c; w_y * s (0 without a twin or a valid label)
    bool live;                           // valid && has
};

__device__ __forceinline__ void m2f_ce_row_twin(CeTwin& k, const CeRow& r, const float* __restrict__ logits, int tr, bool has) {
#pragma clang fp contract(off)
    const int C = r.C;
    float u[16];
    float mu = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        u[c] = (c < C) ? logits[(size_t)tr * C + c] : -INFINITY;
        mu = fmaxf(mu, u[c]);
    }
    // logp_c = (z_c - m) - logf(se), NOT z_c - lse: lse = m + logf(se) is rounded at the size of m, and on saturated rows (|z| in the
    // hundreds) that rounding, harmless to p - onehot in the plain gradient, would be multiplied here by log-ratios of the margin's
    // size.  The twin's logq from its own max and sum in the same way: both lanes of a pair compute the same p, q and ratio bits.
    float su = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) su += (c < C) ? expf(u[c] - mu) : 0.f;
    const float lgs = logf(r.se), lgu = logf(su);
    // e_c = (z_c - u_c) - (z_k - u_k), k the row's own first maximal class: logp_c - logq_c up to a constant.  The gradient needs
    // (logp_c - logq_c) - KL(p || q) = e_c - sum_j p_j e_j; on a confident row (p_k = 1 - tiny) the direct difference of two numbers of
    // the margin's size would lose the tiny part to rounding, while here the j = k term is exactly 0.
    float best = -INFINITY, e0 = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < C && r.z[c] > best) { best = r.z[c]; e0 = r.z[c] - u[c]; }
    }
    float s2 = 0.f;
    k.ebar = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float lp = (c < C) ? ((r.z[c] - r.m) - lgs) : 0.f, lq = (c < C) ? ((u[c] - mu) - lgu) : 0.f;
        k.p[c] = (c < C) ? expf(lp) : 0.f;
        k.q[c] = (c < C) ? expf(lq) : 0.f;
        k.e[c] = (c < C) ? ((r.z[c] - u[c]) - e0) : 0.f;
        k.ebar += k.p[c] * k.e[c];
        s2 += (k.p[c] - k.q[c]) * (lp - lq);
    }
    k.live = r.valid && has;
    k.ws = k.live ? r.wy * (0.5f * s2) : 0.f;
}

// d s / d z_c of the row's own share (without alpha * w_y): p_c * ((logp_c - logq_c) - KL(p || q)) + (p_c - q_c)
__device__ __forceinline__ float m2f_ce_twin_grad(const CeTwin& k, int c) {
#pragma clang fp contract(off)
    return k.live ? (k.p[c] * (k.e[c] - k.ebar) + (k.p[c] - k.q[c])) : 0.f;
}
