// Scoring of one evaluation batch on the device: the criterion's loss, accuracy and weighted F1 by the reference's PER-BATCH rule
// (src/train.py:245-272, src/test.py:51-74: sklearn's accuracy_score / f1_score(average="weighted") on the rows whose label is not -1,
// averaged unweighted over the batches), added into a record that lives in device memory across the batches of a pass.
// Two launches, no float atomics, no memset node: the same bytes on every run, for every grid of the first launch.
//
//   m2f_eval_rows_kernel      one thread per token row (grid-stride): first-max argmax of the C logits, the two criterion terms
//                             (numerator, weight) in exactly m2f_ce_kernel's fp32 arithmetic and operation order (rowops.hip; no
//                             dlogits) into terms[T][2], and the (label, prediction) pair counted into a C x C integer tile in LDS
//                             (integer adds: the counts do not depend on the order).  Each workgroup writes its tile as one partial.
//   m2f_eval_rows_focal_kernel  its focal form (EvalArgs::gamma): the numerator of m2f_ce_focal_kernel, gamma read on the device.
//   m2f_eval_finalize_kernel  one workgroup of 256: the row terms summed in exactly m2f_loss_finalize_kernel's order (thread-strided,
//                             wave sum, (s0 + s1) + (s2 + s3)) - the batch loss num / den has the bits the train path's criterion
//                             gives for the same logits -, the integer partials added, accuracy and weighted F1 in float64, and all
//                             of it ADDED to the record.
//
// Record (M2F_EVAL_RECORD_HEAD doubles, then C x C int64):
//   [0] loss_sum  [1] acc_sum  [2] f1_sum  [3] n_batches  [4] last loss  [5] last accuracy  [6] last weighted F1  [7] unused
//   then cm[true][predicted], the confusion matrix of the whole pass.
// A batch without a labelled row scores NaN three times (0 / 0), as sklearn and torch do; the sums then stay NaN, as the host loop's do.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void m2f_eval_rows_kernel(const EvalArgs a) {
    __shared__ int tile[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    const int C = a.C;
    tile[threadIdx.x] = 0;                                        // (256 threads, 256 cells)
    __syncthreads();
    for (int t = blockIdx.x * 256 + threadIdx.x; t < a.T; t += gridDim.x * 256) {
        // ---- as m2f_ce_kernel, statement for statement ----
        float z[16], w[16];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            z[c] = (c < C) ? a.logits[(size_t)t * C + c] : -INFINITY;
            w[c] = (c < C) ? (a.class_w ? a.class_w[c] : 1.f) : 0.f;
            m = fmaxf(m, z[c]);
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) se += (c < C) ? expf(z[c] - m) : 0.f;
        const float lse = m + logf(se);
        const int64_t y = a.labels[t];
        const bool valid = (y >= 0) && (y < C);
        float wy = 0.f, logpy = 0.f, sm = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < C) {
                const float lp = z[c] - lse;
                sm -= w[c] * lp;
                if (valid && c == (int)y) { wy = w[c]; logpy = lp; }
            }
        }
        const float eps = a.label_smoothing;
        const float num = valid ? ((1.f - eps) * (-logpy) * wy + eps * sm / (float)C) : 0.f;
        a.terms[2 * t] = num;
        a.terms[2 * t + 1] = valid ? wy : 0.f;
        // ---- prediction: the first maximal logit; a NaN counts as maximal (torch.argmax) ----
        float best = z[0];
        int pred = 0;
#pragma unroll
        for (int c = 1; c < 16; ++c) {
            if (c < C && !(best != best) && (z[c] > best || z[c] != z[c])) { best = z[c]; pred = c; }
        }
        if (valid) atomicAdd(&tile[(int)y * C + pred], 1);        // LDS integer add
    }
    __syncthreads();
    if ((int)threadIdx.x < C * C) a.partial[(size_t)blockIdx.x * C * C + threadIdx.x] = tile[threadIdx.x];
}

// The focal form of the rows launch (EvalArgs::gamma non-null): m2f_eval_rows_kernel with the numerator scaled by the focal factor, in
// exactly m2f_ce_focal_kernel<false>'s arithmetic and order (rowops.hip: p = expf(z - lse), omp = the other classes' p added in class
// order, m2f_focal_factor) - validation scores the criterion that trains.  No gradient; argmax and the counts do not depend on gamma.
__global__ __launch_bounds__(256) void m2f_eval_rows_focal_kernel(const EvalArgs a) {
    __shared__ int tile[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    const int C = a.C;
    const float gamma = a.gamma[0];
    tile[threadIdx.x] = 0;                                        // (256 threads, 256 cells)
    __syncthreads();
    for (int t = blockIdx.x * 256 + threadIdx.x; t < a.T; t += gridDim.x * 256) {
        // ---- as m2f_ce_kernel, statement for statement ----
        float z[16], w[16];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            z[c] = (c < C) ? a.logits[(size_t)t * C + c] : -INFINITY;
            w[c] = (c < C) ? (a.class_w ? a.class_w[c] : 1.f) : 0.f;
            m = fmaxf(m, z[c]);
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) se += (c < C) ? expf(z[c] - m) : 0.f;
        const float lse = m + logf(se);
        const int64_t y = a.labels[t];
        const bool valid = (y >= 0) && (y < C);
        float wy = 0.f, logpy = 0.f, sm = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < C) {
                const float lp = z[c] - lse;
                sm -= w[c] * lp;
                if (valid && c == (int)y) { wy = w[c]; logpy = lp; }
            }
        }
        const float eps = a.label_smoothing;
        const float num_ce = valid ? ((1.f - eps) * (-logpy) * wy + eps * sm / (float)C) : 0.f;
        // ---- as m2f_ce_focal_kernel ----
        float omp = 0.f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float p = (c < C) ? expf(z[c] - lse) : 0.f;
            if (c < C && !(valid && c == (int)y)) omp += p;
        }
        const bool focal = gamma > 0.f;
        const float f = m2f_focal_factor(omp, gamma);
        const float num_f = focal ? f * num_ce : num_ce;
        a.terms[2 * t] = valid ? num_f : 0.f;
        a.terms[2 * t + 1] = valid ? wy : 0.f;
        // ---- prediction: the first maximal logit; a NaN counts as maximal (torch.argmax) ----
        float best = z[0];
        int pred = 0;
#pragma unroll
        for (int c = 1; c < 16; ++c) {
            if (c < C && !(best != best) && (z[c] > best || z[c] != z[c])) { best = z[c]; pred = c; }
        }
        if (valid) atomicAdd(&tile[(int)y * C + pred], 1);        // LDS integer add
    }
    __syncthreads();
    if ((int)threadIdx.x < C * C) a.partial[(size_t)blockIdx.x * C * C + threadIdx.x] = tile[threadIdx.x];
}

// The prediction form of the rows launch (EvalArgs::pred non-null): the labels are counted against pred[t] (a decoded path: the Viterbi
// launch of crf.hip in front of it) instead of the row's argmax, and the terms are NOT written - the launch in front (the CRF loss
// without its gradient) left them.  A labelled row without a prediction (pred < 0) is not counted.
__global__ __launch_bounds__(256) void m2f_eval_rows_pred_kernel(const EvalArgs a) {
    __shared__ int tile[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    const int C = a.C;
    tile[threadIdx.x] = 0;
    __syncthreads();
    for (int t = blockIdx.x * 256 + threadIdx.x; t < a.T; t += gridDim.x * 256) {
        const int64_t y = a.labels[t];
        const int pred = a.pred[t];
        if (y >= 0 && y < C && pred >= 0 && pred < C) atomicAdd(&tile[(int)y * C + pred], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < C * C) a.partial[(size_t)blockIdx.x * C * C + threadIdx.x] = tile[threadIdx.x];
}

__global__ __launch_bounds__(256) void m2f_eval_finalize_kernel(const float* __restrict__ terms, int T, int C,
                                                                const int* __restrict__ partial, int n_partial,
                                                                double* __restrict__ record) {
    __shared__ float sn[4], sd[4];
    __shared__ long long cm[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    // ---- as m2f_loss_finalize_kernel ----
    float n = 0.f, dd = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) { n += terms[2 * t]; dd += terms[2 * t + 1]; }
    n = m2f_wave_sum(n);
    dd = m2f_wave_sum(dd);
    if ((threadIdx.x & 63) == 0) { sn[threadIdx.x >> 6] = n; sd[threadIdx.x >> 6] = dd; }
    // ---- the batch's confusion matrix: cell i by thread i ----
    const int cells = C * C;
    long long* __restrict__ total = reinterpret_cast<long long*>(record + M2F_EVAL_RECORD_HEAD);
    if ((int)threadIdx.x < cells) {
        long long s = 0;
        for (int b = 0; b < n_partial; ++b) s += partial[(size_t)b * cells + threadIdx.x];
        cm[threadIdx.x] = s;
        total[threadIdx.x] = total[threadIdx.x] + s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float num = (sn[0] + sn[1]) + (sn[2] + sn[3]);
    const float den = (sd[0] + sd[1]) + (sd[2] + sd[3]);
    const float loss = num / den;
    long long rows = 0, trace = 0;
    for (int i = 0; i < cells; ++i) rows += cm[i];
    double f1w = 0.0;
    for (int c = 0; c < C; ++c) {
        long long support = 0, predicted = 0;
        for (int j = 0; j < C; ++j) { support += cm[c * C + j]; predicted += cm[j * C + c]; }
        trace += cm[c * C + c];
        const long long d = support + predicted;
        const double f = d ? (double)(2 * cm[c * C + c]) / (double)d : 0.0;
        f1w += f * (double)support;
    }
    const double acc = (double)trace / (double)rows;             // 0 / 0 = NaN for a batch without a labelled row
    const double f1 = f1w / (double)rows;
    record[0] = record[0] + (double)loss;
    record[1] = record[1] + acc;
    record[2] = record[2] + f1;
    record[3] = record[3] + 1.0;
    record[4] = (double)loss;
    record[5] = acc;
    record[6] = f1;
}

}  // namespace

hipError_t m2f_launch_eval_scores(const EvalArgs& a, double* record, hipStream_t stream) {
    if (!a.logits || !a.labels || !a.terms || !a.partial || !record || a.T < 1 || a.C < 1 || a.C > M2F_EVAL_MAX_C)
        return hipErrorInvalidValue;
    const int blocks = m2f_eval_blocks(a.T);
    if (a.pred) hipLaunchKernelGGL(m2f_eval_rows_pred_kernel, dim3(blocks), dim3(256), 0, stream, a);
    else if (a.gamma) hipLaunchKernelGGL(m2f_eval_rows_focal_kernel, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(m2f_eval_rows_kernel, dim3(blocks), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(m2f_eval_finalize_kernel, dim3(1), dim3(256), 0, stream, a.terms, a.T, a.C, a.partial, blocks, record);
    return hipGetLastError();
}
