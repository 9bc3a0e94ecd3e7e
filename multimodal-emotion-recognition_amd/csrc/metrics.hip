// Scoring of one evaluation batch on the device: the criterion's loss, accuracy and weighted F1 by the reference's PER-BATCH rule
// (src/train.py:245-272, src/test.py:51-74: sklearn's accuracy_score / f1_score(average="weighted") on the rows whose label is not -1,
// averaged unweighted over the batches), added into a record that lives in device memory across the batches of a pass.
// Two launches, no float atomics, no memset node: the same bytes on every run, for every grid of the first launch.
//
//   m2f_eval_rows_kernel<FOCAL>  one thread per token row (grid-stride): first-max argmax of the C logits, the two criterion terms
//                             (numerator, weight) by criterion_row.h's helpers - the train criterion's own statements, without
//                             dlogits - into terms[T][2], and the (label, prediction) pair counted into a C x C integer tile in LDS
//                             (integer adds: the counts do not depend on the order).  Each workgroup writes its tile as one partial.
//                             FOCAL (EvalArgs::gamma): the focal criterion's numerator, gamma read on the device.
//   m2f_eval_finalize_kernel  one workgroup of 256: the row terms summed by m2f_block_sum_terms, as the train criterion's finalize
//                             launch sums them - the batch loss num / den has the bits the train path's criterion gives for the
//                             same logits -, the integer partials added, accuracy and weighted F1 in float64, and all of it ADDED
//                             to the record.
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
#include "criterion_row.h"

#pragma clang fp contract(off)

namespace {

// FOCAL (EvalArgs::gamma non-null): the numerator scaled by the focal factor, gamma read on the device - validation scores the criterion
// that trains.  No gradient; argmax and the counts do not depend on gamma.
template <bool FOCAL>
__global__ __launch_bounds__(256) void m2f_eval_rows_kernel(const EvalArgs a) {
    __shared__ int tile[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    const int C = a.C;
    float gamma = 0.f;
    if constexpr (FOCAL) gamma = a.gamma[0];
    tile[threadIdx.x] = 0;                                        // (256 threads, 256 cells)
    __syncthreads();
    for (int t = blockIdx.x * 256 + threadIdx.x; t < a.T; t += gridDim.x * 256) {
        CeRow r;
        m2f_ce_row_forward(r, a.logits, a.labels, a.class_w, a.label_smoothing, t, C);
        if constexpr (FOCAL) {
            CeFocal f;
            m2f_ce_row_focal(f, r, gamma);
            a.terms[2 * t] = r.valid ? f.num_f : 0.f;
        } else {
            a.terms[2 * t] = r.num;
        }
        a.terms[2 * t + 1] = r.valid ? r.wy : 0.f;
        // ---- prediction: the first maximal logit; a NaN counts as maximal (torch.argmax) ----
        float best = r.z[0];
        int pred = 0;
#pragma unroll
        for (int c = 1; c < 16; ++c) {
            if (c < C && !(best != best) && (r.z[c] > best || r.z[c] != r.z[c])) { best = r.z[c]; pred = c; }
        }
        if (r.valid) atomicAdd(&tile[(int)r.y * C + pred], 1);    // LDS integer add
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
    __shared__ long long cm[M2F_EVAL_MAX_C * M2F_EVAL_MAX_C];
    // ---- the batch's confusion matrix: cell i by thread i ----
    const int cells = C * C;
    long long* __restrict__ total = reinterpret_cast<long long*>(record + M2F_EVAL_RECORD_HEAD);
    if ((int)threadIdx.x < cells) {
        long long s = 0;
        for (int b = 0; b < n_partial; ++b) s += partial[(size_t)b * cells + threadIdx.x];
        cm[threadIdx.x] = s;
        total[threadIdx.x] = total[threadIdx.x] + s;
    }
    // ---- the row terms, summed as the train criterion's finalize launch sums them (its barrier also publishes cm) ----
    float s[2];
    m2f_block_sum_terms<2>(terms, T, s);
    if (threadIdx.x != 0) return;
    const float num = s[0], den = s[1];
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
    else if (a.gamma) hipLaunchKernelGGL(m2f_eval_rows_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(m2f_eval_rows_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(m2f_eval_finalize_kernel, dim3(1), dim3(256), 0, stream, a.terms, a.T, a.C, a.partial, blocks, record);
    return hipGetLastError();
}
