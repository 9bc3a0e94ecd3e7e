// Per-tensor statistics and histograms of one flat buffer in the model's parameter layout (parameters, gradients, moments, the EMA;
// fp32 or bf16), or of the difference a - b of two fp32 buffers: what wandb.watch(model, log="all") logs per parameter tensor, taken
// where the values live.  Three launches, no float atomics: every byte of the record is the same on every run and for every grid.
//
//   m2f_tstats_partial_kernel   pass 1: one StatPartial per SLICE (ops.h ParamSlice: at most M2F_PARAM_SLICE consecutive elements of
//                               ONE tensor - the array gradnorm.hip walks; tag = the tensor's index; the pads between tensors belong to no slice
//                               and are never read).  NaN / inf / zero counts, min and max of the finite values, their sum and sum of
//                               squares in float64 (one FMA per element, as gradnorm.hip's square16).  A partial depends on its slice
//                               alone: lane t takes the same elements in the same order whichever workgroup picks the slice up.
//   m2f_tstats_finalize_kernel  one workgroup per tensor (grid-stride): the tensor's partials combined in a fixed order (thread t takes
//                               slices t, t + 256, ... in slice order; then a fixed tree) into the tensor's record row; the row's bin
//                               counts zeroed; *den_ptr into the record header.
//   m2f_tstats_hist_kernel      pass 2, a second read (a tensor's range exists only after pass 1): `bins` equal-width bins over
//                               [lo, hi] = the row's finite min / max, torch.histc's rule in IEEE fp32, operation for operation:
//                               pos = (int)((x - lo) * bins / (hi - lo)), bins -> bins - 1.  Counts are integers: LDS counters per
//                               workgroup, flushed with 64-bit integer adds into the row when the workgroup's run of slices leaves
//                               the tensor - integer sums do not depend on order, so neither on the grid.
//
// The LDS counters: gradients pile up in a few middle bins, and 64 lanes adding to ONE LDS word serialise.  The bin array is therefore
// kept SIXTEEN times, the copy chosen by lane & 15, laid out bin-major (word = bin * 16 + copy): the sixteen copies of one bin sit in
// sixteen different banks, so lanes that hit the same bin spread over sixteen words and at most four lanes (64 / 16) share a word even
// when the whole buffer is one constant.  (Copy-major, word = copy * bins + bin, would put every copy of a bin into the SAME bank for
// bins = 64 or 256: different words, same bank - as slow as one word.)  16 x 256 x 4 B = 16 KB at the most.  A reduction inside the
// wave before the add (match-any on the bin) was the alternative; it costs a data-dependent loop per element where this costs one LDS
// add, and it was not needed to keep the pass on the memory side.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "ops.h"

namespace {

constexpr int SLICE = M2F_PARAM_SLICE;
constexpr int COPIES = 16;

__device__ __forceinline__ float bf16_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }
__device__ __forceinline__ bool finite32(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7F800000u) != 0x7F800000u; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ u32x4 load16(const void* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else return *reinterpret_cast<const u32x4*>(p);
}

// the values of sixteen bytes, in element order: f(x, k) with k = element index & 1 (a compile-time constant after unrolling)
template <bool A16, bool DIFF, class F>
__device__ __forceinline__ void each16(const u32x4& r, const u32x4& q, F& f) {
    if constexpr (A16) {
        f(bf16_lo(r.x), 0); f(bf16_hi(r.x), 1); f(bf16_lo(r.y), 0); f(bf16_hi(r.y), 1);
        f(bf16_lo(r.z), 0); f(bf16_hi(r.z), 1); f(bf16_lo(r.w), 0); f(bf16_hi(r.w), 1);
    } else {
        const f32x4 a = __builtin_bit_cast(f32x4, r);
        if constexpr (DIFF) {
            const f32x4 b = __builtin_bit_cast(f32x4, q);
            f(a[0] - b[0], 0); f(a[1] - b[1], 1); f(a[2] - b[2], 0); f(a[3] - b[3], 1);      // x = a - b: one fp32 subtraction
        } else {
            f(a[0], 0); f(a[1], 1); f(a[2], 0); f(a[3], 1);
        }
    }
}

template <bool A16, bool DIFF>
__device__ __forceinline__ float value1(const void* a, const float* b, long long o) {
    if constexpr (A16) return __builtin_bit_cast(float, (uint32_t)static_cast<const uint16_t*>(a)[o] << 16);
    else if constexpr (DIFF) return static_cast<const float*>(a)[o] - b[o];
    else return static_cast<const float*>(a)[o];
}

// Every element of slice `sl` that lane `tid` of a 256-lane workgroup owns, in a fixed order: 16-byte loads (4 fp32 / 8 bf16 values),
// round j at element (j * 256 + tid) * V.  A whole slice issues every load first; the short last slice of a tensor reads nothing at or
// beyond element n (whole vectors while they fit, then single elements).  DIFF (fp32 only): x = a - b.
template <bool A16, bool DIFF, bool NT, class F>
__device__ __forceinline__ void slice_values(const void* a, const float* b, const ParamSlice& sl, int tid, F& f) {
    constexpr int V = A16 ? 8 : 4;
    constexpr int ROUNDS = SLICE / (256 * V);
    constexpr int ESZ = A16 ? 2 : 4;
    const char* abase = static_cast<const char*>(a) + sl.off * ESZ;              // tensor offsets are multiples of 64 elements: 16-byte aligned
    const char* bbase = DIFF ? reinterpret_cast<const char*>(b + sl.off) : nullptr;
    if (sl.n == SLICE) {
        u32x4 r[ROUNDS], q[DIFF ? ROUNDS : 1];
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            r[j] = load16<NT>(abase + ((size_t)j * 256 + tid) * 16);
            if constexpr (DIFF) q[j] = load16<NT>(bbase + ((size_t)j * 256 + tid) * 16);
        }
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) each16<A16, DIFF>(r[j], q[DIFF ? j : 0], f);
    } else {
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const int e = (j * 256 + tid) * V;
            if (e + V <= sl.n) {
                const u32x4 r = load16<NT>(abase + (size_t)e * ESZ);
                u32x4 q = {0u, 0u, 0u, 0u};
                if constexpr (DIFF) q = load16<NT>(bbase + (size_t)e * ESZ);
                each16<A16, DIFF>(r, q, f);
            } else {
                for (int k = e; k < sl.n; ++k) f(value1<A16, DIFF>(a, b, sl.off + k), 0);
            }
        }
    }
}

__device__ __forceinline__ double shfl_xor_d(double x, int o) { return __shfl_xor(x, o, 64); }

struct WaveStat { double sum, sumsq; float mn, mx; int nan, inf, zeros; };

// ---- pass 1 ----------------------------------------------------------------------------------------------------------------------
template <bool A16, bool DIFF, bool NT>
__global__ __launch_bounds__(256) void m2f_tstats_partial_kernel(const void* __restrict__ a, const float* __restrict__ b,
                                                                  const ParamSlice* __restrict__ slices, int ns,
                                                                  StatPartial* __restrict__ partial) {
    __shared__ WaveStat red[2][4];
    const int tid = threadIdx.x;
    int par = 0;
    for (int s = (int)blockIdx.x; s < ns; s += (int)gridDim.x, par ^= 1) {
        const ParamSlice sl = slices[s];
        double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
        float mn = __builtin_inff(), mx = -__builtin_inff();
        int n_nan = 0, n_inf = 0, n_zero = 0;
        auto take = [&](float x, int k) {
            const bool fin = finite32(x);
            const bool inf = (__builtin_bit_cast(uint32_t, x) & 0x7FFFFFFFu) == 0x7F800000u;
            n_inf += inf;
            n_nan += !fin && !inf;
            n_zero += x == 0.0f;
            mn = fin ? fminf(mn, x) : mn;
            mx = fin ? fmaxf(mx, x) : mx;
            const double d = fin ? x : 0.0f;                                   // (a non-finite value adds 0 and 0 * 0)
            if (k) { s1 += d; q1 = __builtin_fma(d, d, q1); }
            else   { s0 += d; q0 = __builtin_fma(d, d, q0); }
        };
        slice_values<A16, DIFF, NT>(a, b, sl, tid, take);
        double sum = s0 + s1, sumsq = q0 + q1;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {                                   // butterfly: the same order in every wave of every run
            sum += shfl_xor_d(sum, o);
            sumsq += shfl_xor_d(sumsq, o);
            mn = fminf(mn, __shfl_xor(mn, o, 64));
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            n_nan += __shfl_xor(n_nan, o, 64);
            n_inf += __shfl_xor(n_inf, o, 64);
            n_zero += __shfl_xor(n_zero, o, 64);
        }
        if ((tid & 63) == 0) red[par][tid >> 6] = WaveStat{sum, sumsq, mn, mx, n_nan, n_inf, n_zero};
        __syncthreads();                                                       // (red[par ^ 1] is free again after this barrier)
        if (tid == 0) {
            WaveStat t = red[par][0];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const WaveStat u = red[par][w];
                t.sum += u.sum; t.sumsq += u.sumsq; t.mn = fminf(t.mn, u.mn); t.mx = fmaxf(t.mx, u.mx);
                t.nan += u.nan; t.inf += u.inf; t.zeros += u.zeros;
            }
            StatPartial p;
            p.sum = t.sum; p.sumsq = t.sumsq; p.mn = t.mn; p.mx = t.mx; p.nan = t.nan; p.inf = t.inf; p.zeros = t.zeros; p.pad_ = 0;
            partial[s] = p;
        }
    }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------------------
struct TensorStat { double sum, sumsq, numel, nan, inf, zeros; float mn, mx; };      // (counts as float64: exact far beyond 2^31)

__device__ __forceinline__ void fold(TensorStat& t, const TensorStat& u) {
    t.sum += u.sum; t.sumsq += u.sumsq; t.numel += u.numel; t.nan += u.nan; t.inf += u.inf; t.zeros += u.zeros;
    t.mn = fminf(t.mn, u.mn); t.mx = fmaxf(t.mx, u.mx);
}

__global__ __launch_bounds__(256) void m2f_tstats_finalize_kernel(const StatPartial* __restrict__ partial, const ParamSlice* __restrict__ slices,
                                                                   const int* __restrict__ tensor_begin, int n_tensors, int bins,
                                                                   const float* __restrict__ den_ptr, double* __restrict__ record) {
    __shared__ TensorStat red[4];
    const int tid = threadIdx.x;
    const int row_len = M2F_TSTATS_FIELDS + bins;
    if (blockIdx.x == 0 && tid == 0) {
        record[0] = den_ptr ? (double)*den_ptr : 1.0;
        record[1] = (double)n_tensors;
        record[2] = (double)bins;
        record[3] = 0.0;
    }
    for (int t = (int)blockIdx.x; t < n_tensors; t += (int)gridDim.x) {
        TensorStat a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inff(), -__builtin_inff()};
        for (int s = tensor_begin[t] + tid; s < tensor_begin[t + 1]; s += 256) {
            const StatPartial p = partial[s];
            const TensorStat u = {p.sum, p.sumsq, (double)slices[s].n, (double)p.nan, (double)p.inf, (double)p.zeros, p.mn, p.mx};
            fold(a, u);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            TensorStat u;
            u.sum = shfl_xor_d(a.sum, o); u.sumsq = shfl_xor_d(a.sumsq, o); u.numel = shfl_xor_d(a.numel, o);
            u.nan = shfl_xor_d(a.nan, o); u.inf = shfl_xor_d(a.inf, o); u.zeros = shfl_xor_d(a.zeros, o);
            u.mn = __shfl_xor(a.mn, o, 64); u.mx = __shfl_xor(a.mx, o, 64);
            fold(a, u);
        }
        if ((tid & 63) == 0) red[tid >> 6] = a;
        __syncthreads();
        double* row = record + M2F_TSTATS_HEADER + (size_t)t * row_len;
        if (tid == 0) {
            TensorStat r = red[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) fold(r, red[w]);
            const double finite = r.numel - r.nan - r.inf;
            const bool any = finite > 0.0;
            const double nan = __builtin_nan("");
            row[0] = r.numel; row[1] = finite; row[2] = r.nan; row[3] = r.inf; row[4] = r.zeros;
            row[5] = any ? (double)r.mn : nan; row[6] = any ? (double)r.mx : nan;
            row[7] = any ? r.sum : nan; row[8] = any ? r.sumsq : nan;
        }
        long long* counts = reinterpret_cast<long long*>(row + M2F_TSTATS_FIELDS);
        for (int i = tid; i < bins; i += 256) counts[i] = 0;
        __syncthreads();                                                       // (red is read above and written by the next tensor)
    }
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------------------
// Workgroup w takes the slices [w * per, (w + 1) * per): consecutive slices are mostly of one tensor, so the LDS counters are flushed
// once per tensor the run touches, not once per slice.
template <bool A16, bool DIFF, bool NT>
__global__ __launch_bounds__(256) void m2f_tstats_hist_kernel(const void* __restrict__ a, const float* __restrict__ b,
                                                               const ParamSlice* __restrict__ slices, int ns, int per, int bins,
                                                               double* __restrict__ record) {
    __shared__ int h[256 * COPIES];
    const int tid = threadIdx.x;
    const int copy = tid & (COPIES - 1);
    const int row_len = M2F_TSTATS_FIELDS + bins;
    for (int i = tid; i < bins * COPIES; i += 256) h[i] = 0;
    __syncthreads();
    const int s_begin = (int)blockIdx.x * per;
    const int s_end = s_begin + per < ns ? s_begin + per : ns;
    const float binsf = (float)bins;
    int cur = -1;
    bool live = false;
    float lo = 0.f, width = 1.f;
    auto flush = [&](int t) {
        __syncthreads();
        if (tid < bins) {                                                      // bins <= 256 = the workgroup
            int c = 0;
#pragma unroll
            for (int k = 0; k < COPIES; ++k) { c += h[tid * COPIES + k]; h[tid * COPIES + k] = 0; }
            if (c) {
                unsigned long long* counts = reinterpret_cast<unsigned long long*>(record + M2F_TSTATS_HEADER + (size_t)t * row_len + M2F_TSTATS_FIELDS);
                atomicAdd(counts + tid, (unsigned long long)c);                // integer add: the total does not depend on who adds first
            }
        }
        __syncthreads();
    };
    for (int s = s_begin; s < s_end; ++s) {
        const ParamSlice sl = slices[s];
        if (sl.tag != cur) {                                                // block-uniform
            if (cur >= 0 && live) flush(cur);
            cur = sl.tag;
            const double* row = record + M2F_TSTATS_HEADER + (size_t)cur * row_len;
            live = row[1] > 0.0;                                               // a tensor with no finite value: zero counts
            lo = (float)row[5];                                                // (fp32 values widened by the finalize launch: exact)
            float hi = (float)row[6];
            if (lo == hi) { lo = lo - 1.0f; hi = hi + 1.0f; }
            width = hi - lo;
        }
        if (!live) continue;
        auto bin = [&](float x, int) {
            if (finite32(x)) {
                int pos = (int)((x - lo) * binsf / width);                     // IEEE fp32, in this order; the division is correctly rounded
                pos = pos < 0 ? 0 : (pos > bins - 1 ? bins - 1 : pos);         // pos == bins -> bins - 1; nothing leaves the array
                atomicAdd(&h[pos * COPIES + copy], 1);
            }
        };
        slice_values<A16, DIFF, NT>(a, b, sl, tid, bin);
    }
    if (cur >= 0 && live) flush(cur);
}

}  // namespace

hipError_t m2f_launch_tensor_stats(const void* a, int a_is_bf16, const float* b, const ParamSlice* slices, const int* tensor_begin,
                                   int n_slices, int n_tensors, int bins, const float* den_ptr, StatPartial* partial, double* record,
                                   int grid, int nontemporal, int passes, hipStream_t stream) {
    if (!a || !slices || !tensor_begin || !partial || !record || n_slices < 0 || n_tensors < 0 || bins < 2 || bins > M2F_TSTATS_MAX_BINS || !(passes & 3) ||
        (a_is_bf16 && b) || (reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(b) & 15) ||
        (reinterpret_cast<uintptr_t>(partial) & 7) || (reinterpret_cast<uintptr_t>(record) & 7))
        return hipErrorInvalidValue;
    // memory-bound: at most 2,048 workgroups (the grid decides who takes a slice, never what comes out)
    const int want = grid > 0 ? grid : 2048;
    const int blocks = want < n_slices ? want : n_slices;
    const int per = blocks > 0 ? (n_slices + blocks - 1) / blocks : 1;
    const int hblocks = blocks > 0 ? (n_slices + per - 1) / per : 0;
#define M2F_TS_LAUNCH(A16, DIFF, NT)                                                                                                    \
    do {                                                                                                                                \
        if (blocks > 0 && (passes & 1))                                                                                                 \
            hipLaunchKernelGGL((m2f_tstats_partial_kernel<A16, DIFF, NT>), dim3(blocks), dim3(256), 0, stream, a, b, slices, n_slices,  \
                               partial);                                                                                                \
        if (passes & 1)                                                                                                                 \
            hipLaunchKernelGGL(m2f_tstats_finalize_kernel, dim3(n_tensors < 1024 ? (n_tensors > 0 ? n_tensors : 1) : 1024), dim3(256), 0,  \
                           stream, partial, slices, tensor_begin, n_tensors, bins, den_ptr, record);                                    \
        if (hblocks > 0 && (passes & 2))                                                                                                \
            hipLaunchKernelGGL((m2f_tstats_hist_kernel<A16, DIFF, NT>), dim3(hblocks), dim3(256), 0, stream, a, b, slices, n_slices,    \
                               per, bins, record);                                                                                      \
    } while (0)
    if (a_is_bf16)  { if (nontemporal) M2F_TS_LAUNCH(true, false, true);  else M2F_TS_LAUNCH(true, false, false); }
    else if (b)     { if (nontemporal) M2F_TS_LAUNCH(false, true, true);  else M2F_TS_LAUNCH(false, true, false); }
    else            { if (nontemporal) M2F_TS_LAUNCH(false, false, true); else M2F_TS_LAUNCH(false, false, false); }
#undef M2F_TS_LAUNCH
    return hipGetLastError();
}
