// Stream and chunk plans (include/m2fnet_hip.h): plans of plan.h whose attention sites run the streaming kernels against per-slot K / V caches
// or page pools - their life cycle, m2f_stream_step / m2f_stream_prefill, and snapshot gather / scatter of live dialogues through a plan.
#include "plan.h"

using namespace m2f;

extern "C" {

/* One plan object, over dense caches (n_pages == 0) or page pools; sizing and creation below serve the four public entry points.  The
   paged ones hand a page count below 1 on as -1, so that it is refused here, in its place among the other checks. */
static m2f_plan* stream_plan_new(const m2f_config* cfg, int S, int& C, int past, int precision, int n_pages, int page_rows) {
    if (precision != M2F_F32 && precision != M2F_BF16) { fail("bad precision"); return nullptr; }
    if (n_pages) {
        if (page_rows != 16 && page_rows != 32 && page_rows != 64) { fail("paged stream plan: page_rows must be 16, 32 or 64 (got " + std::to_string(page_rows) + ")"); return nullptr; }
        if (n_pages < 1) { fail("paged stream plan: n_pages >= 1 required"); return nullptr; }
    }
    if (!cfg || S < 1) { fail("stream plan: S >= 1 stream slots required"); return nullptr; }
    if (past >= 0 && C < past + 1) C = past + 1;
    if (C < 1 || C > M2F_ATTN_STREAM_MAX_C) {
        fail("stream plan: capacity must be 1 .. " + std::to_string(M2F_ATTN_STREAM_MAX_C) + " rows per slot (got " + std::to_string(C) +
             "; a window of `past` utterances needs past + 1)");
        return nullptr;
    }
    m2f_config c = *cfg;
    c.dropout = 0.f;                                    // an eval plan: no dropout site
    m2f_plan* p = plan_new(&c, S, 1, precision, 0);
    if (!p) return nullptr;
    const int hmax = std::max(c.audio_enabled ? c.d_audio / std::max(c.nhead_audio, 1) : 0,
                              std::max(c.text_enabled ? c.d_text / std::max(c.nhead_text, 1) : 0, c.fam_enabled ? c.d_fam / std::max(c.nhead_fam, 1) : 0));
    if (hmax > 128) { fail("stream plan: head dims up to 128 (got " + std::to_string(hmax) + ")"); delete p; return nullptr; }
    p->streaming = true; p->s_cap = C; p->s_ring = past >= 0;
    p->band_past = past < 0 ? -1 : past; p->band_future = 0;       // (what m2f_plan_get_attention_band reports)
    if (n_pages) {
        p->s_pages = n_pages;
        p->s_pg.R = page_rows; p->s_pg.tw = (C + page_rows - 1) / page_rows; p->s_pg.n_pages = n_pages;
    }
    return p;
}
static int64_t stream_workspace_bytes(const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows, int shared) {
    int64_t need = -1;
    return size_and_build(stream_plan_new(cfg, S, C, past, precision, n_pages, page_rows), shared != 0, 4096, nullptr, need) == BUILD_OK ? need : -1;
}
// a stream or chunk plan `p` (null: refused by its maker) bound to its buffers and built through the one size-then-build path; `dry`: its twin
static m2f_plan* stream_build(m2f_plan* p, m2f_plan* dry, float* params, void* workspace, int64_t workspace_bytes, uint16_t* param_shadow) {
    if (!p) { delete dry; return nullptr; }
    p->ext_wshadow = param_shadow;
    p->params = params; p->grads = nullptr; p->rng = nullptr;
    p->ws_base = static_cast<char*>(workspace); p->ws_bytes = workspace_bytes;
    int64_t need = -1;
    const BuildStatus st = size_and_build(dry, param_shadow != nullptr, 4096, p, need);
    if (st == BUILD_TOO_SMALL) fail("workspace too small: need " + std::to_string(need) + " bytes");
    if (st != BUILD_OK) { delete p; return nullptr; }
    return p;
}
static m2f_plan* stream_plan_create(const char* who, const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows,
                                    float* params, void* workspace, int64_t workspace_bytes, uint16_t* param_shadow) {
    if (!params || !workspace) { fail("params / workspace must not be NULL"); return nullptr; }
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(params) & 255) || (reinterpret_cast<uintptr_t>(param_shadow) & 255)) {
        fail("params / workspace / param_shadow must be 256-byte aligned"); return nullptr;
    }
    m2f_plan* p = stream_build(stream_plan_new(cfg, S, C, past, precision, n_pages, page_rows), stream_plan_new(cfg, S, C, past, precision, n_pages, page_rows),
                               params, workspace, workspace_bytes, param_shadow);
    if (!p) return nullptr;
    // counters and table start at zero whatever the workspace held (page 0 is a valid id; an entry is read only once the host has set it)
    if (hipMemset(p->s_len, 0, (size_t)S * sizeof(int)) != hipSuccess || hipMemset(p->s_active, 0, (size_t)S) != hipSuccess ||
        (n_pages && hipMemset(p->bufs[M2F_BUF_STREAM_TABLE], 0, (size_t)S * p->s_pg.tw * sizeof(int)) != hipSuccess)) {
        fail(std::string(who) + ": hipMemset"); delete p; return nullptr;
    }
    return p;
}
int64_t m2f_stream_workspace_bytes(const m2f_config* cfg, int S, int C, int past, int precision, int shared) {
    return stream_workspace_bytes(cfg, S, C, past, precision, 0, 0, shared);
}
m2f_plan* m2f_plan_create_stream(const m2f_config* cfg, int S, int C, int past, int precision, float* params, void* workspace,
                                 int64_t workspace_bytes, uint16_t* param_shadow) {
    return stream_plan_create("m2f_plan_create_stream", cfg, S, C, past, precision, 0, 0, params, workspace, workspace_bytes, param_shadow);
}
int64_t m2f_stream_paged_workspace_bytes(const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows, int shared) {
    return stream_workspace_bytes(cfg, S, C, past, precision, n_pages < 1 ? -1 : n_pages, page_rows, shared);
}
m2f_plan* m2f_plan_create_stream_paged(const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows, float* params,
                                       void* workspace, int64_t workspace_bytes, uint16_t* param_shadow) {
    return stream_plan_create("m2f_plan_create_stream_paged", cfg, S, C, past, precision, n_pages < 1 ? -1 : n_pages, page_rows, params, workspace,
                              workspace_bytes, param_shadow);
}
// The CRF's forward filter (m2f_plan_stream_crf): behind the classifier, in FRONT of the launch that advances the counters - it reads
// the counts the slots held before this call.  rows: 1 (step: one row per active slot) or the chunk (prefill: n_new[s] rows in order).
static int stream_filter(m2f_plan& P, int rows, hipStream_t s) {
    if (!P.s_phi) return 0;
    CrfFilterArgs a;
    a.logits = static_cast<const float*>(P.bufs[M2F_BUF_LOGITS]); a.S = P.B; a.C = P.cfg.cls_out; a.rows = rows;
    a.params = P.crit.crf_params; a.count = P.s_len; a.active = rows == 1 ? P.s_active : nullptr; a.n_new = rows == 1 ? nullptr : P.s_new;
    a.phi = P.s_phi;
    M2F_HIP(m2f_launch_crf_filter(a, s));
    return 0;
}
int m2f_plan_stream_crf(m2f_plan* plan, const float* params, float* phi) {
    if (!plan) return fail("m2f_plan_stream_crf: NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.streaming && !P.s_parent) return fail("m2f_plan_stream_crf needs a stream or chunk plan (m2f_plan_create_stream / m2f_plan_create_stream_chunk)");
    if ((params == nullptr) != (phi == nullptr)) return fail("m2f_plan_stream_crf: params and phi come together (both NULL: off)");
    if (params && (P.cfg.cls_out < 2 || P.cfg.cls_out > 16)) return fail("m2f_plan_stream_crf: 2 .. 16 classes");
    if ((reinterpret_cast<uintptr_t>(params) & 15) || (reinterpret_cast<uintptr_t>(phi) & 3)) return fail("m2f_plan_stream_crf: params must be 16-byte aligned");
    if (params == P.crit.crf_params && phi == P.s_phi) return 0;
    // the filter launch travels by value inside the captured step / prefill: the capture goes, one eager call comes first
    M2F_HIP(hipDeviceSynchronize());
    P.graphs[P.s_parent ? SLOT_PREFILL : SLOT_STREAM].reset();
    ++P.generation;
    P.warmed = false;
    P.crit.crf_params = params; P.s_phi = phi;
    return 0;
}
static int stream_body(m2f_plan& P, hipStream_t s) {
    if (int r = do_forward(P, s)) return r;
    if (int r = stream_filter(P, 1, s)) return r;
    if (P.spk_same | P.spk_other)          // speaker heads: the new ids into the rows the new utterances took, behind the step's last attention launch
        M2F_HIP(m2f_launch_stream_advance_speakers(P.s_len, P.s_active, P.B, P.s_spk, static_cast<const uint8_t*>(P.bufs[M2F_BUF_SPEAKERS]), P.s_cap, P.s_ring, s));
    else
        M2F_HIP(m2f_launch_stream_advance(P.s_len, P.s_active, P.B, s));
    return 0;
}
int m2f_stream_step(m2f_plan* plan, int use_graph, m2f_stream_t stream) {
    if (!plan) return fail("m2f_stream_step: NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.streaming || P.s_parent) return fail("m2f_stream_step needs a stream plan (m2f_plan_create_stream)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!use_graph || !P.warmed) { P.warmed = true; return stream_body(P, s); }
    return replay_slot(P.graphs[SLOT_STREAM], GraphKey::forward(P.params_fresh, P.generation), s, [&] { return stream_body(P, s); });
}
int m2f_stream_reset(m2f_plan* plan, const uint8_t* slot_mask, m2f_stream_t stream) {
    if (!plan) return fail("m2f_stream_reset: NULL plan (destroyed?)");
    if (!plan->streaming || plan->s_parent) return fail("m2f_stream_reset needs a stream plan (m2f_plan_create_stream)");
    M2F_HIP(m2f_launch_stream_reset(plan->s_len, slot_mask, plan->B, static_cast<hipStream_t>(stream)));
    return 0;
}
int64_t m2f_stream_cache_bytes(m2f_plan* plan) { return plan && plan->streaming && !plan->s_parent ? plan->s_cache_bytes : -1; }     // (a chunk plan owns no cache)

/* Snapshot / restore of a stream plan's dialogues.  See include/m2fnet_hip.h and stream_cache.hip. */
static void stream_sites(const m2f_plan& P, std::vector<StreamCacheSite>& sites, std::vector<int>* hds, int& rowv) {
    const int bf16 = P.prec == M2F_PREC_BF16;
    rowv = 0;
    for (const Launch& l : P.built.fwd) {
        if (l.kind != OP_ATTN_FWD) continue;
        for (int i = 0; i < l.sb.count; ++i) {
            const AttnStreamProblem& q = l.sb.pr[i];
            const int vpr = m2f_stream_cache_row_vecs(q.hd, bf16);
            sites.push_back({q.kcache, q.vcache, q.H, vpr, rowv, 0});
            if (hds) hds->push_back(q.hd);
            rowv += 2 * q.H * vpr;
        }
    }
}
int64_t m2f_stream_snapshot_row_elems(m2f_plan* plan) {
    if (!plan || !plan->streaming || plan->s_parent) { fail("m2f_stream_snapshot_row_elems needs a stream plan (m2f_plan_create_stream)"); return -1; }
    std::vector<StreamCacheSite> sites;
    int rowv = 0;
    stream_sites(*plan, sites, nullptr, rowv);
    return (int64_t)rowv * (plan->prec == M2F_PREC_BF16 ? 8 : 4);
}
int m2f_stream_snapshot_sites(m2f_plan* plan, int* H, int* hd, int max_sites) {
    if (!plan || !plan->streaming || plan->s_parent) return fail("m2f_stream_snapshot_sites needs a stream plan (m2f_plan_create_stream)");
    std::vector<StreamCacheSite> sites;
    std::vector<int> hds;
    int rowv = 0;
    stream_sites(*plan, sites, &hds, rowv);
    for (size_t i = 0; i < sites.size() && (int)i < max_sites; ++i) {
        if (H) H[i] = sites[i].H;
        if (hd) hd[i] = hds[i];
    }
    return (int)sites.size();
}
static int stream_cache_move(m2f_plan* plan, const char* who, int n, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets,
                             void* packed, int64_t packed_elems, int scatter, m2f_stream_t stream) {
    const std::string w(who);
    if (!plan) return fail(w + ": NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.streaming || P.s_parent) return fail(w + " needs a stream plan (m2f_plan_create_stream)");
    if (n < 0 || packed_elems < 0) return fail(w + ": n, packed_elems >= 0 required");
    if (n == 0) return 0;
    if (!slots || !lengths || !row_offsets || !packed) return fail(w + ": NULL argument");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(w + ": the packed buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(row_offsets) & 7) return fail(w + ": row_offsets must be 8-byte aligned");
    std::vector<StreamCacheSite> sites;
    int rowv = 0;
    stream_sites(P, sites, nullptr, rowv);
    if (sites.empty()) return fail(w + ": the plan has no attention site");
    const int epv = P.prec == M2F_PREC_BF16 ? 8 : 4;            // elements per 16-byte vector
    for (size_t s0 = 0; s0 < sites.size(); s0 += M2F_STREAM_CACHE_MAX_SITES) {
        StreamCacheBatch cb;
        memset(&cb, 0, sizeof(cb));
        cb.count = (int)std::min(sites.size() - s0, (size_t)M2F_STREAM_CACHE_MAX_SITES);
        for (int i = 0; i < cb.count; ++i) cb.site[i] = sites[s0 + i];
        cb.S = P.B; cb.C = P.s_cap; cb.rowv = rowv; cb.n_entries = n;
        cb.slots = slots; cb.lengths = lengths; cb.row_offsets = row_offsets;
        cb.packed = packed; cb.packed_vecs = packed_elems / epv; cb.len = P.s_len;
        M2F_HIP(m2f_launch_stream_cache(cb, P.s_pages ? &P.s_pg : nullptr, scatter, static_cast<hipStream_t>(stream)));
    }
    return 0;
}
int m2f_stream_gather(m2f_plan* plan, int n, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets, void* packed,
                      int64_t packed_elems, m2f_stream_t stream) {
    return stream_cache_move(plan, "m2f_stream_gather", n, slots, lengths, row_offsets, packed, packed_elems, 0, stream);
}
int m2f_stream_scatter(m2f_plan* plan, int n, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets, const void* packed,
                       int64_t packed_elems, m2f_stream_t stream) {
    return stream_cache_move(plan, "m2f_stream_scatter", n, slots, lengths, row_offsets, const_cast<void*>(packed), packed_elems, 1, stream);
}

/* Attention rows of a stream plan's steps.  See include/m2fnet_hip.h, attention_stream.hip (the weights-emitting form) and attention_weights.hip. */
int64_t m2f_stream_attention_elems(m2f_plan* plan) {
    if (!plan || !plan->streaming || plan->s_parent) { fail("m2f_stream_attention_elems needs a stream plan (m2f_plan_create_stream)"); return -1; }
    int64_t n = 0;
    for (const AttnSiteRef& a : plan->built.attn_sites) n += (int64_t)plan->B * a.H * plan->s_cap;
    return n;
}
int m2f_plan_stream_attention(m2f_plan* plan, float* buffer, int64_t buffer_elems) {
    if (!plan) return fail("m2f_plan_stream_attention: NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.streaming || P.s_parent) return fail("m2f_plan_stream_attention needs a stream plan (m2f_plan_create_stream); the chunk kernel has no weights form");
    if (buffer == P.s_attn) return 0;
    if (buffer && ((reinterpret_cast<uintptr_t>(buffer) & 15) || buffer_elems < m2f_stream_attention_elems(plan)))
        return fail("m2f_plan_stream_attention: the buffer must be 16-byte aligned and hold m2f_stream_attention_elems() floats");
    // site k's rows start S * C * (heads of the sites before it) floats in; a launch's problem is found through the probabilities
    // buffer the eval plan gave it (one per site)
    std::vector<Launch>& fwd = P.built.fwd;
    for (Launch& l : fwd) {
        if (l.kind != OP_ATTN_FWD) continue;
        memset(&l.sw, 0, sizeof(l.sw));
        l.sw_on = false;
        if (!buffer) continue;
        for (int i = 0; i < l.sb.count; ++i) {
            int64_t off = 0;
            bool found = false;
            for (const AttnSiteRef& a : P.built.attn_sites) {
                if (a.probs == l.ab.pr[i].probs) { found = true; break; }
                off += (int64_t)P.B * a.H * P.s_cap;
            }
            if (!found) return fail("m2f_plan_stream_attention: an attention launch holds a site the plan does not list");
            l.sw.w[i] = buffer + off;
        }
        l.sw_on = true;
    }
    // the launches travel by value inside the captured step and run another kernel from here on: the capture goes, one eager step comes first
    M2F_HIP(hipDeviceSynchronize());
    P.graphs[SLOT_STREAM].reset();
    ++P.generation;
    P.warmed = false;
    P.s_attn = buffer;
    P.bufs[M2F_BUF_STREAM_ATTN] = buffer;
    return 0;
}
int m2f_stream_attention(m2f_plan* plan, const int* sites, int n_sites, int per_head, float* const* out, m2f_stream_t stream) {
    if (!plan) return fail("m2f_stream_attention: NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.streaming || P.s_parent) return fail("m2f_stream_attention needs a stream plan (m2f_plan_create_stream)");
    if (!P.s_attn) return fail("m2f_stream_attention: attention rows are off (m2f_plan_stream_attention)");
    if (n_sites < 0 || (n_sites > 0 && (!sites || !out))) return fail("m2f_stream_attention: NULL argument");
    const std::vector<AttnSiteRef>& all = P.built.attn_sites;
    std::vector<int64_t> offs(all.size() + 1, 0);
    for (size_t k = 0; k < all.size(); ++k) offs[k + 1] = offs[k] + (int64_t)P.B * all[k].H * P.s_cap;
    for (int i = 0; i < n_sites; ++i)
        if (sites[i] < 0 || sites[i] >= (int)all.size() || !out[i]) return fail("m2f_stream_attention: a site outside the plan's list, or a NULL output");
    for (int s0 = 0; s0 < n_sites; s0 += M2F_ATTN_WEIGHTS_MAX_SITES) {
        AttnWeightsBatch wb;
        memset(&wb, 0, sizeof(wb));
        wb.count = std::min(n_sites - s0, M2F_ATTN_WEIGHTS_MAX_SITES);
        for (int i = 0; i < wb.count; ++i) {
            const AttnSiteRef& a = all[sites[s0 + i]];
            wb.site[i] = {P.s_attn + offs[sites[s0 + i]], out[s0 + i], a.H, 1.0f / (float)a.H};
        }
        wb.B = P.B; wb.L = P.s_cap; wb.per_head = per_head != 0;
        M2F_HIP(m2f_launch_attn_weight_rows(wb, static_cast<hipStream_t>(stream)));
    }
    return 0;
}

/* Chunk plans.  See include/m2fnet_hip.h. */
static m2f_plan* chunk_plan_new(m2f_plan* parent, int T) {
    if (!parent || !parent->streaming || parent->s_parent) { fail("chunk plan: the parent must be a stream plan (m2f_plan_create_stream)"); return nullptr; }
    if (T < 2 || T > M2F_ATTN_STREAM_MAX_CHUNK) {
        fail("chunk plan: 2 .. " + std::to_string(M2F_ATTN_STREAM_MAX_CHUNK) + " rows per slot and call (got " + std::to_string(T) + ")");
        return nullptr;
    }
    m2f_plan* p = plan_new(&parent->cfg, parent->B, T, parent->prec, 0);      // (the parent's configuration: dropout already 0)
    if (!p) return nullptr;
    p->streaming = true; p->s_cap = parent->s_cap; p->s_ring = parent->s_ring;
    p->band_past = parent->band_past; p->band_future = parent->band_future;
    p->bias_gain = parent->bias_gain;                                          // (the chunk's sites take it when they are built)
    p->spk_same = parent->spk_same; p->spk_other = parent->spk_other; p->s_spk = parent->s_spk;      // (likewise, through apply_speakers)
    p->s_parent = parent; p->s_chunk = T;
    p->s_pages = parent->s_pages; p->s_pg = parent->s_pg;                      // (a paged parent: the same pools through the same table)
    return p;
}
int64_t m2f_stream_chunk_workspace_bytes(m2f_plan* parent, int T, int shared) {
    int64_t need = -1;
    return size_and_build(chunk_plan_new(parent, T), shared != 0, 4096, nullptr, need) == BUILD_OK ? need : -1;
}
m2f_plan* m2f_plan_create_stream_chunk(m2f_plan* parent, int T, float* params, void* workspace, int64_t workspace_bytes,
                                       uint16_t* param_shadow) {
    if (!params || !workspace) { fail("params / workspace must not be NULL"); return nullptr; }
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(params) & 255) || (reinterpret_cast<uintptr_t>(param_shadow) & 255)) {
        fail("params / workspace / param_shadow must be 256-byte aligned"); return nullptr;
    }
    m2f_plan* p = stream_build(chunk_plan_new(parent, T), chunk_plan_new(parent, T), params, workspace, workspace_bytes, param_shadow);
    if (!p) return nullptr;
    if (hipMemset(p->s_new, 0, (size_t)p->B * sizeof(int)) != hipSuccess) { fail("m2f_plan_create_stream_chunk: hipMemset"); delete p; return nullptr; }
    return p;
}
static int prefill_body(m2f_plan& P, hipStream_t s) {
    if (int r = do_forward(P, s)) return r;
    if (int r = stream_filter(P, P.s_chunk, s)) return r;
    if (P.spk_same | P.spk_other)          // (as the step: the chunk's ids, then the counters)
        M2F_HIP(m2f_launch_stream_advance_speakers_n(P.s_len, P.s_new, P.B, P.s_chunk, P.s_spk, static_cast<const uint8_t*>(P.bufs[M2F_BUF_SPEAKERS]), P.s_cap, P.s_ring, s));
    else
        M2F_HIP(m2f_launch_stream_advance_n(P.s_len, P.s_new, P.B, P.s_chunk, s));
    return 0;
}
int m2f_stream_prefill(m2f_plan* plan, int use_graph, m2f_stream_t stream) {
    if (!plan) return fail("m2f_stream_prefill: NULL plan (destroyed?)");
    m2f_plan& P = *plan;
    if (!P.s_parent) return fail("m2f_stream_prefill needs a chunk plan (m2f_plan_create_stream_chunk)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!use_graph || !P.warmed) { P.warmed = true; return prefill_body(P, s); }
    return replay_slot(P.graphs[SLOT_PREFILL], GraphKey::forward(P.params_fresh, P.generation), s, [&] { return prefill_body(P, s); });
}

}  // extern "C"
