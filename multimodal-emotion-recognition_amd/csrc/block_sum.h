// The float64 workgroup sum of the gradient-norm and SAM finalize kernels (gradnorm.hip, sam.hip), written once: both records of one
// buffer carry the same sqrt(sum of squares) because both sums ARE this tree.
#pragma once
#include <hip/hip_runtime.h>

// butterfly over the 64 lanes: every lane ends with the same sum, formed in the same order
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// workgroup sum of one double per lane: wave shuffle tree, then the WAVES wave sums through LDS, added in wave order by thread 0.
// `red` = WAVES doubles the caller does not touch until its next barrier.  The result is valid in thread 0 only.
template <int WAVES>
__device__ __forceinline__ double block_sum(double x, double* red) {
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += red[w];
    }
    return s;
}
