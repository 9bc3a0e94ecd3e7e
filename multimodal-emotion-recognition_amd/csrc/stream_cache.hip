// Snapshot and restore of the streaming K / V caches on gfx950: the live cache rows of listed stream slots <-> one packed buffer.
//
// A dialogue's whole state under a causal context band is the K and V rows its slot holds at every attention site plus its length
// (attention_stream.hip has the cache layouts); the rows never change once written.  GATHER copies the live rows of `n_entries` listed
// slots out of the caches into a packed buffer, SCATTER copies a packed buffer into the rows of listed slots and sets their lengths.
//
// PACKED LAYOUT.  Entry e holds the rows_e = min(lengths[e], C) live PHYSICAL rows 0 .. rows_e - 1 of slot slots[e] (a ring keeps its
// phase), laid out as the dense cache with C replaced by rows_e:
//     [site in table order][K, V][H][rows_e][pad(hd)]
// and starts at element row_offsets[e] * W of the buffer, W = sum over sites of 2 * H * pad(hd).  Pad columns travel as they are.  A row
// is a whole number of 16-byte vectors at every site and in both precisions, so every segment starts 16-byte aligned and the kernels
// move bytes: the element type never enters (a site's row is `vpr` vectors wide).
//
// One launch serves every site and every listed slot: blockIdx.y = entry, blockIdx.x = (site, K / V, head) segment, found through a
// by-value site table.  A workgroup moves its segment's rows_e * vpr vectors: contiguous on the packed side, and on the cache side one
// contiguous run (dense) or one run per page (paged: the slot's page ids are fetched once into LDS and clamped to the pool, as in the
// paged attention kernels).  16-byte accesses, U independent loads issued before their stores, 64-bit offsets, no atomics.  Rows
// >= rows_e of a slot, other slots and other pages are never written.  In a scatter one lane per entry also stores len[slot] = length
// (an ordinary store; an entry of length 0 therefore resets its slot).
// An entry whose slot, length or offset is out of range (slot outside 0 .. S - 1, negative length or offset, rows past the end of the
// packed buffer) is skipped whole: device-side arrays can never send an access outside the buffers the launch was given.
#include "common.h"
#include "ops.h"
#include "attn_stream_rows.h"

namespace {

template <bool PAGED, bool SCATTER>
__global__ __launch_bounds__(256) void m2f_stream_cache_kernel(const StreamCacheBatch cb, const AttnStreamPaging pg) {
    constexpr int U = 4;                          // vectors in flight per lane: their loads are issued together
    __shared__ int spg[32];                       // paged: the slot's page ids, entry p = logical rows p*R .. p*R + R - 1

    const int e = cb.e0 + blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
    const int slot = cb.slots[e], length = cb.lengths[e];
    const long long ro = cb.row_offsets[e];
    if (slot < 0 || slot >= cb.S || length < 0 || ro < 0) return;                       // (uniform: the whole workgroup leaves)
    const int rows = length < cb.C ? length : cb.C;
    if ((ro + rows) * (long long)cb.rowv > cb.packed_vecs) return;
    if (SCATTER && seg == 0 && tid == 0) cb.len[slot] = length;
    if (rows == 0) return;

    int si = 0;
    while (si + 1 < cb.count && seg >= cb.sb[si + 1]) ++si;
    const StreamCacheSite& st = cb.site[si];
    const int local = seg - cb.sb[si];            // 0 .. 2H - 1: K heads, then V heads
    const int H = st.H, vpr = st.vpr;
    const int kv = local >= H ? 1 : 0, h = local - kv * H;
    u32x4* cache = static_cast<u32x4*>(kv ? st.vcache : st.kcache);
    u32x4* packed = static_cast<u32x4*>(cb.packed) + (size_t)ro * (size_t)cb.rowv + (size_t)rows * (size_t)(st.colv + local * vpr);
    const int nv = rows * vpr;                    // (<= 512 rows * 32 vectors)

    int runv = 0;                                 // paged: vectors of one page's rows of one head
    size_t page_stride = 0;
    if (PAGED) {
        m2f_stream_page_ids(spg, pg, slot, rows, tid);          // (one 4-byte load per page that holds a row of the entry)
        __syncthreads();
        runv = vpr << pg.lgR;
        page_stride = (size_t)H * (size_t)runv;
        cache += (size_t)h * (size_t)runv;        // this head's rows of page 0
    } else {
        cache += ((size_t)slot * H + h) * (size_t)cb.C * (size_t)vpr;
    }
    auto at = [&](int i) -> u32x4* {              // vector i of the segment on the cache side
        if (!PAGED) return cache + i;
        const int run = i / runv;
        return cache + (size_t)spg[run] * page_stride + (size_t)(i - run * runv);
    };

    for (int i0 = tid; i0 < nv; i0 += 256 * U) {
        u32x4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            if (i < nv) x[u] = SCATTER ? packed[i] : *at(i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            if (i < nv) {
                if (SCATTER) *at(i) = x[u];
                else packed[i] = x[u];
            }
        }
    }
}

}  // namespace

int m2f_stream_cache_row_vecs(int hd, int bf16) {
    return m2f_stream_hdp(hd, bf16 != 0) / (bf16 ? 8 : 4);
}

// cb.site[i].colv and cb.rowv are the caller's (a launch may serve a slice of a longer site list); sb, e0 are filled here.
hipError_t m2f_launch_stream_cache(StreamCacheBatch& cb, const AttnStreamPaging* paging, int scatter, hipStream_t stream) {
    if (cb.count < 1 || cb.count > M2F_STREAM_CACHE_MAX_SITES || cb.S < 1 || cb.C < 1 || cb.C > M2F_ATTN_STREAM_MAX_C || cb.n_entries < 0)
        return hipErrorInvalidValue;
    if (!cb.slots || !cb.lengths || !cb.row_offsets || !cb.packed || cb.packed_vecs < 0 || cb.rowv < 1 || (scatter && !cb.len)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(cb.packed) & 15) || (reinterpret_cast<uintptr_t>(cb.row_offsets) & 7)) return hipErrorInvalidValue;
    AttnStreamPaging pg = {nullptr, 0, 0, 0, 0};
    if (paging) {
        pg = *paging;
        AttnStreamBatch ab{};                     // (the check reads the capacity alone)
        ab.C = cb.C;
        if (!m2f_attn_stream_paging_ok(ab, pg)) return hipErrorInvalidValue;
    }
    int segs = 0;
    for (int i = 0; i < M2F_STREAM_CACHE_MAX_SITES; ++i) cb.sb[i] = 0x7fffffff;
    for (int i = 0; i < cb.count; ++i) {
        const StreamCacheSite& s = cb.site[i];
        if (s.H < 1 || s.vpr < 1 || s.vpr > 32 || s.colv < 0 || s.colv + 2 * s.H * s.vpr > cb.rowv || !s.kcache || !s.vcache) return hipErrorInvalidValue;
        if ((reinterpret_cast<uintptr_t>(s.kcache) & 15) || (reinterpret_cast<uintptr_t>(s.vcache) & 15)) return hipErrorInvalidValue;
        cb.sb[i] = segs;
        segs += 2 * s.H;
    }
    for (int e0 = 0; e0 < cb.n_entries; e0 += 65535) {          // (blockIdx.y carries the entry)
        cb.e0 = e0;
        const int ne = cb.n_entries - e0 < 65535 ? cb.n_entries - e0 : 65535;
        const dim3 grid(segs, ne), block(256);
        if (paging) {
            if (scatter) hipLaunchKernelGGL((m2f_stream_cache_kernel<true, true>), grid, block, 0, stream, cb, pg);
            else hipLaunchKernelGGL((m2f_stream_cache_kernel<true, false>), grid, block, 0, stream, cb, pg);
        } else {
            if (scatter) hipLaunchKernelGGL((m2f_stream_cache_kernel<false, true>), grid, block, 0, stream, cb, pg);
            else hipLaunchKernelGGL((m2f_stream_cache_kernel<false, false>), grid, block, 0, stream, cb, pg);
        }
        if (hipError_t err = hipGetLastError()) return err;
    }
    return hipSuccess;
}
