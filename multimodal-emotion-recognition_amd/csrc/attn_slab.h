// Slab staging and the exact-fp32 MFMA step shared by the dialogue attention kernels (attention.hip: L <= 64, one workgroup
// per (dialogue, head); attention_dlong.hip: L <= 512, one workgroup per 64-row block).  Included inside an anonymous
// namespace by each translation unit.
#pragma once


constexpr int NTHR = 256;          // 4 wavefronts per (dialogue, head)
constexpr int NWAVE = NTHR / 64;

// [Lp x W] zero-padded LDS copy of src rows [0, L) x cols [0, hd), generic form (any size / alignment).  Loads are
// UNCONDITIONAL (clamped address + select) and issued in batches before any LDS write (guarded loads compile to
// branch + s_waitcnt vmcnt(0) each).
__device__ __forceinline__ void load_slab(float* __restrict__ lds, int ld, int Lp, int W,
                                          const float* __restrict__ src, int ldg, int L, int hd, int tid) {
    const int total = Lp * W;
#pragma unroll 1
    for (int base = 0; base < total; base += NTHR * 4) {
        float x[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = base + tid + NTHR * u;
            const int r = e / W, c = e - r * W;
            const bool ok = e < total && r < L && c < hd;
            off[u] = e < total ? r * ld + c : -1;
            x[u] = src[ok ? (size_t)r * ldg + c : (size_t)0];
            if (!ok) x[u] = 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) lds[off[u]] = x[u];
    }
}

// Fast form for slabs of at most NTHR*NV float4 whose rows are 16-byte aligned: the (row, column) of each of a thread's
// (up to) NV float4 is worked out ONCE (one integer division) and shared by every slab of the kernel (same L, hd, W),
// all slabs are issued before the first is committed.  NV = 2 * (Lp / 16) covers every head dim <= 128, so the generic
// (scalar, division-heavy) form below only serves unaligned operands; it is kept small on purpose.
template <int NV>
struct SlabGeom {
    int goff_rc[NV];     // r * 65536 + c   (r < 64, c < 256)
    int loff[NV];        // r * ld + c  (LDS float offset)
    bool inb[NV];        // element index < total (a slot of this thread exists)
    bool ok[NV];         // ... and lies inside [0, L) x [0, hd)
};
template <int NV>
__device__ __forceinline__ void slab_geom(SlabGeom<NV>& G, int L, int hd, int Lp, int W, int ld, int tid) {
    const int C4 = W >> 2, total = Lp * C4;
    int r = tid / C4, c4 = tid - r * C4;
    const int dr = NTHR / C4, dc = NTHR - dr * C4;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int e = tid + NTHR * u;
        const int c = c4 << 2;
        G.inb[u] = e < total;
        G.ok[u] = G.inb[u] && r < L && c < hd;
        G.goff_rc[u] = (r << 16) | c;
        G.loff[u] = r * ld + c;
        r += dr; c4 += dc;
        if (c4 >= C4) { c4 -= C4; ++r; }
    }
}
template <int NV>
__device__ __forceinline__ bool slab_fast_ok(const float* src, int ldg, int hd, int Lp, int W) {
    return ((hd & 3) == 0) && ((ldg & 3) == 0) && ((reinterpret_cast<uintptr_t>(src) & 15) == 0) && (Lp * (W >> 2) <= NTHR * NV);
}
template <int NV>
struct SlabRegs { f32x4 x[NV]; uint32_t w0[NV], w1[NV]; };     // w0 / w1: the raw 4 bf16 of a chunk staged from a shadow
template <int NV>
__device__ __forceinline__ void slab_issue(SlabRegs<NV>& R, const SlabGeom<NV>& G, const float* __restrict__ src, int ldg) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int r = G.goff_rc[u] >> 16, c = G.goff_rc[u] & 0xFFFF;
        const uint32_t o = G.ok[u] ? (uint32_t)(r * ldg + c) * 4u : 0u;
        R.x[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(src) + (size_t)o);
    }
}
// bf16 mode: the same slab from the operand's bf16 SHADOW (same element index; the producer wrote both copies): half the bytes
// of the kernels' dominant cost - at C3 a merged encoder launch of the backward kernel read 37 MB of fp32 slabs.  The raw
// 8 bytes (4 bf16) wait in w0 / w1 until slab_value() widens them (exact: bf16 -> fp32 is a shift).
template <int NV>
__device__ __forceinline__ void slab_issue16(SlabRegs<NV>& R, const SlabGeom<NV>& G, const uint16_t* __restrict__ src, int ldg) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int r = G.goff_rc[u] >> 16, c = G.goff_rc[u] & 0xFFFF;
        const uint32_t o = G.ok[u] ? (uint32_t)(r * ldg + c) * 2u : 0u;
        const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(src) + (size_t)o);
        R.w0[u] = w.x; R.w1[u] = w.y;
    }
}
template <int NV>
__device__ __forceinline__ f32x4 slab_value(const SlabRegs<NV>& R, int u, bool from16) {
    if (!from16) return R.x[u];
    const uint32_t a = R.w0[u], b = R.w1[u];
    const f32x4 v = {__builtin_bit_cast(float, a << 16), __builtin_bit_cast(float, a & 0xFFFF0000u),
                     __builtin_bit_cast(float, b << 16), __builtin_bit_cast(float, b & 0xFFFF0000u)};
    return v;
}

template <int NV>
__device__ __forceinline__ void slab_commit(const SlabRegs<NV>& R, const SlabGeom<NV>& G, float* __restrict__ lds, bool from16 = false) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        if (G.inb[u]) {
            const bool ok = G.ok[u];
            const f32x4 v = slab_value(R, u, from16);
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            f32x2* d = reinterpret_cast<f32x2*>(lds + G.loff[u]);          // r*(W+2) + c is even: 8-byte aligned
            d[0] = f32x2{ok ? v[0] : 0.f, ok ? v[1] : 0.f};
            d[1] = f32x2{ok ? v[2] : 0.f, ok ? v[3] : 0.f};
        }
    }
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
