// What the streaming kernel files (attention_stream.hip, attention_stream_chunk.hip, stream_cache.hip) share about a cache row: its
// padded width, the 16-byte access of one lane, and where logical row j of a slot lives in a page pool.
#pragma once
#include "common.h"
#include "ops.h"

// the head dim padded to a 16-byte multiple: 4 floats (fp32 caches) or 8 bf16 values (bf16 caches)
__host__ __device__ inline int m2f_stream_hdp(int hd, bool bf16) { return bf16 ? (hd + 7) & ~7 : (hd + 3) & ~3; }

template <bool BF16> struct Row;
template <> struct Row<false> {
    static constexpr int EPL = 4;                 // elements per lane and 16-byte access
    typedef float elem_t;
    __device__ static __forceinline__ void load(const elem_t* p, float (&x)[4]) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    }
    __device__ static __forceinline__ void store(elem_t* p, const float (&x)[4]) {
        const f32x4 v = {x[0], x[1], x[2], x[3]};
        *reinterpret_cast<f32x4*>(p) = v;
    }
};
template <> struct Row<true> {
    static constexpr int EPL = 8;
    typedef uint16_t elem_t;
    __device__ static __forceinline__ void load(const elem_t* p, float (&x)[8]) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __builtin_bit_cast(float, v[i] << 16);
            x[2 * i + 1] = __builtin_bit_cast(float, v[i] & 0xffff0000u);
        }
    }
    __device__ static __forceinline__ void store(elem_t* p, const float (&x)[8]) {       // (x: already bf16 values)
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (uint32_t)m2f_bf16_bits(x[2 * i]) | ((uint32_t)m2f_bf16_bits(x[2 * i + 1]) << 16);
        *reinterpret_cast<u32x4*>(p) = v;
    }
};

// Paged addressing.  The workgroup fetches its slot's page ids ONCE - thread e loads table entry e (<= 32 entries: 512 rows of 16-row
// pages) into spg[32] in LDS - and every row address takes the id from there: no dependent global load per row.  Only the entries of
// the pages that hold one of the slot's first `rows` logical rows are loaded; entries behind that are never dereferenced, whatever they
// hold.  An id is clamped to the pool (0 .. n_pages - 1): a torn table reads the wrong page, never unmapped memory.  The caller's
// barrier publishes spg.
__device__ __forceinline__ void m2f_stream_page_ids(int* spg, const AttnStreamPaging& pg, int slot, int rows, int tid) {
    if (tid < 32) {
        int id = 0;
        if (tid < ((rows + (1 << pg.lgR) - 1) >> pg.lgR)) id = pg.table[(size_t)slot * pg.tw + tid];
        spg[tid] = min(max(id, 0), pg.n_pages - 1);
    }
}
// logical row j of the slot, column c -> element offset from the head's row 0 of page 0; page_stride: elements of one page, all heads
__device__ __forceinline__ size_t m2f_stream_row_off(const int* spg, int lgR, size_t page_stride, int j, int hdp, int c = 0) {
    return (size_t)spg[j >> lgR] * page_stride + (size_t)((j & ((1 << lgR) - 1)) * hdp + c);
}
