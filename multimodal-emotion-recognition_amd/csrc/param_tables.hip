// The per-tensor tables of a configuration and the entry points that walk the flat parameter buffer tensor by tensor: the parameter
// shadows' table region, the Adam steps over ranges and groups, the EMA exchange, the gradient norm and the model watch's statistics.
// Every fact has one home: param_table (the host table of a configuration - the size queries, the table region, plan_build.hip's coverage
// walk and every device table derive from it), cut_slices, tensor_range (checked on the host table before any device call) and
// device_table (the one cache of device copies).
#include "param_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

namespace m2f {

namespace { thread_local std::string g_err; }
int fail(const std::string& m) { g_err = m; return 1; }
int hipfail(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return 2;
}
const char* last_error() { return g_err.c_str(); }
int ema_args_bad(const char* what, const float* ema, float ema_w) {
    if (!ema || (reinterpret_cast<uintptr_t>(ema) & 15)) return fail(std::string(what) + ": a 16-byte aligned EMA buffer is required");
    if (!(ema_w >= 0.f && ema_w <= 1.f)) return fail(std::string(what) + ": ema_w = 1 - decay must lie in [0, 1]");
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// parameter map
// ---------------------------------------------------------------------------------------------------
namespace {
size_t pm_add(ParamMap& pm, size_t n, int rows = 0, int cols = 0) {
    const size_t off = pm.total;
    pm.offsets.push_back((int64_t)off);
    pm.numels.push_back((int64_t)n);
    pm.total = (off + n + 63) / 64 * 64;
    if (rows > 0 && cols > 0) {
        const size_t so = pm.shadow_elems;
        pm.shadow_elems += ((size_t)rows * ((cols + 7) & ~7) + 63) / 64 * 64;
        pm.mats.push_back({off, rows, cols, so, pm.shadow_elems});
        pm.shadow_elems += ((size_t)cols * ((rows + 7) & ~7) + 63) / 64 * 64;
    }
    return off;
}

void pm_modality(ParamMap& pm, ModalityP& m, int d, int ntrans, int nlayers, int dff, int dfam) {
    m.enc.resize(ntrans);
    for (int e = 0; e < ntrans; ++e) {
        for (int l = 0; l < nlayers; ++l) {
            EncLayerP p;
            p.in_w = pm_add(pm, (size_t)3 * d * d, 3 * d, d);
            p.in_b = pm_add(pm, (size_t)3 * d);
            p.out_w = pm_add(pm, (size_t)d * d, d, d);
            p.out_b = pm_add(pm, d);
            p.l1_w = pm_add(pm, (size_t)dff * d, dff, d);
            p.l1_b = pm_add(pm, dff);
            p.l2_w = pm_add(pm, (size_t)d * dff, d, dff);
            p.l2_b = pm_add(pm, d);
            p.n1_w = pm_add(pm, d);
            p.n1_b = pm_add(pm, d);
            p.n2_w = pm_add(pm, d);
            p.n2_b = pm_add(pm, d);
            m.enc[e].push_back(p);
        }
        if (e == 0) {                       // the final norm object is shared by all encoders of a modality
            m.norm_w = pm_add(pm, d);
            m.norm_b = pm_add(pm, d);
        }
    }
    m.proj_w = pm_add(pm, (size_t)dfam * d, dfam, d);
    m.proj_b = pm_add(pm, dfam);
}
}  // namespace

int cls_in_width(const m2f_config& c) { return (c.audio_enabled && c.text_enabled) ? 2 * c.d_fam : c.d_fam; }

int check_config(const m2f_config& c) {
    if (!c.audio_enabled && !c.text_enabled) return fail("At least one of audio and text must be enabled!");
    if (c.fam_enabled && !(c.audio_enabled && c.text_enabled))
        return fail("Fusion Attention Module can only be used with both audio and text enabled!");
    if (c.audio_enabled && (c.nhead_audio < 1 || c.d_audio % c.nhead_audio)) return fail("AUDIO: embed_dim must be divisible by num_heads");
    if (c.text_enabled && (c.nhead_text < 1 || c.d_text % c.nhead_text)) return fail("TEXT: embed_dim must be divisible by num_heads");
    if (c.fam_enabled && (c.nhead_fam < 1 || c.d_fam % c.nhead_fam)) return fail("FAM: embed_dim must be divisible by num_heads");
    if (c.cls_out < 1 || c.cls_out > 16) return fail("CLASSIFIER.output_size must be in [1,16]");
    if (c.dropout < 0.f || c.dropout >= 1.f) return fail("dropout must be in [0,1)");
    if (c.dim_ff < 1 || c.cls_hidden < 1 || c.d_fam < 1) return fail("bad widths");
    const int dmax = std::max(std::max(c.audio_enabled ? c.d_audio : 0, c.text_enabled ? c.d_text : 0), c.d_fam);
    if (dmax > 2048) return fail("embedding sizes above 2048 are not supported by the LayerNorm kernels");
    return 0;
}

int build_param_map(const m2f_config& c, ParamMap& pm) {
    if (check_config(c)) return 1;
    if (c.audio_enabled) pm_modality(pm, pm.audio, c.d_audio, c.ntrans_audio, c.nlayers_audio, c.dim_ff, c.d_fam);
    if (c.text_enabled) pm_modality(pm, pm.text, c.d_text, c.ntrans_text, c.nlayers_text, c.dim_ff, c.d_fam);
    if (c.fam_enabled) {
        const size_t E = c.d_fam;
        for (int i = 0; i < c.nlayers_fam; ++i) {
            FamP f;
            f.in_w = pm_add(pm, 3 * E * E, (int)(3 * E), (int)E);
            f.in_b = pm_add(pm, 3 * E);
            f.out_w = pm_add(pm, E * E, (int)E, (int)E);
            f.out_b = pm_add(pm, E);
            f.lin_w = pm_add(pm, E * 2 * E, (int)E, (int)(2 * E));
            f.lin_b = pm_add(pm, E);
            pm.fam.push_back(f);
        }
    }
    const size_t h = c.cls_hidden, in = cls_in_width(c);
    LinP l0;
    l0.w = pm_add(pm, h * in, (int)h, (int)in);
    l0.b = pm_add(pm, h);
    pm.cls.push_back(l0);
    for (int j = 0; j < std::max(c.cls_layers - 2, 0); ++j) {
        LinP l;
        l.w = pm_add(pm, h * h, (int)h, (int)h);
        l.b = pm_add(pm, h);
        pm.cls.push_back(l);
    }
    LinP ll;
    ll.w = pm_add(pm, (size_t)c.cls_out * h, c.cls_out, (int)h);
    ll.b = pm_add(pm, c.cls_out);
    pm.cls.push_back(ll);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// the host table and what is cut from it
// ---------------------------------------------------------------------------------------------------
int item_tiles(const AdamItem& it, bool flat) {
    if (it.rows > 0 && !flat) return ((it.rows + 63) / 64) * it.tiles_c;
    const long long n = it.rows > 0 ? (long long)it.rows * it.cols : (long long)it.cols;
    return (int)((n + 4095) / 4096);
}

int retile(std::vector<AdamItem>& items, std::vector<int>* groups, bool flat, std::vector<int>& tile_begin) {
    if (groups) {
        size_t kept = 0;
        for (size_t i = 0; i < items.size(); ++i)
            if ((*groups)[i] >= 0) { items[kept] = items[i]; (*groups)[kept++] = (*groups)[i]; }
        items.resize(kept); groups->resize(kept);
    }
    tile_begin.clear();
    int tiles = 0;
    for (AdamItem& it : items) {
        it.tile_begin = tiles;
        tile_begin.push_back(tiles);
        tiles += item_tiles(it, flat);
    }
    tile_begin.push_back(tiles);
    return tiles;
}

namespace {
std::mutex g_mu;                              // the host tables and the device tables
std::vector<const ParamTable*> g_host_tables;

int build_param_table(const m2f_config& cfg, ParamTable& t) {
    ParamMap pm;
    if (build_param_map(cfg, pm)) return 1;
    t.cfg = cfg;
    t.offsets = pm.offsets; t.numels = pm.numels; t.total = pm.total;
    t.shadow_elems = (pm.shadow_elems + 64 + 127) / 128 * 128;
    size_t mi = 0;
    int tiles = 0, slices = 0;
    for (size_t i = 0; i < pm.offsets.size(); ++i) {
        AdamItem it; memset(&it, 0, sizeof(it));
        it.off = pm.offsets[i]; it.tile_begin = tiles;
        if (mi < pm.mats.size() && pm.mats[mi].off == (size_t)pm.offsets[i]) {
            const ParamMap::Mat& m = pm.mats[mi++];
            it.rows = m.rows; it.cols = m.cols; it.soff = (long long)m.soff; it.soff_t = (long long)m.soff_t;
            it.tiles_c = (m.cols + 63) / 64;
        } else {
            const int64_t next = i + 1 < pm.offsets.size() ? pm.offsets[i + 1] : (int64_t)pm.total;
            it.rows = 0; it.cols = (int)(next - pm.offsets[i]);            // the tensor and its pad up to the next one (multiples of 64)
            it.tiles_c = 1;
        }
        t.tile_begin.push_back(tiles);
        t.slice_begin.push_back(slices);
        t.items.push_back(it);
        tiles += item_tiles(it);
        slices += (int)((pm.numels[i] + M2F_PARAM_SLICE - 1) / M2F_PARAM_SLICE);
    }
    t.tile_begin.push_back(tiles);
    t.slice_begin.push_back(slices);
    if (mi != pm.mats.size()) return fail("adam_table: parameter map walk lost a matrix");
    t.items_fit = t.items.size() <= M2F_ADAM_MAX_ITEMS &&
                  t.items.size() * sizeof(AdamItem) + t.tile_begin.size() * sizeof(int) <= (size_t)ADAM_TABLE_BYTES;
    return 0;
}
}  // namespace

const ParamTable* param_table(const m2f_config& cfg, bool need_items) {
    const ParamTable* t = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        for (const ParamTable* h : g_host_tables)
            if (memcmp(&h->cfg, &cfg, sizeof(m2f_config)) == 0) { t = h; break; }
        if (!t) {
            std::unique_ptr<ParamTable> made(new ParamTable);
            if (build_param_table(cfg, *made)) return nullptr;
            g_host_tables.push_back(t = made.release());
        }
    }
    if (need_items && !t->items_fit) { fail("too many parameter tensors for the fused optimizer table"); return nullptr; }
    return t;
}

int tensor_at(const ParamTable& t, long long e) {
    return (int)(std::upper_bound(t.offsets.begin(), t.offsets.end(), (int64_t)e) - t.offsets.begin()) - 1;
}

int upload_packed(void*& dev, const std::vector<std::pair<const void*, size_t>>& sec, std::vector<char*>& at) {
    size_t bytes = 0;
    for (const auto& x : sec) bytes = ((bytes + 255) & ~(size_t)255) + x.second;
    if (dev) { (void)hipFree(dev); dev = nullptr; }
    M2F_HIP(hipMalloc(&dev, bytes + 256));
    at.assign(1, static_cast<char*>(dev));
    for (size_t i = 0; i < sec.size(); ++i) {
        M2F_HIP(hipMemcpy(at[i], sec[i].first, sec[i].second, hipMemcpyHostToDevice));
        at.push_back(at[i] + ((sec[i].second + 255) & ~(size_t)255));
    }
    return 0;
}

int group_map_bad(const char* what, const ParamTable& t, const int* tensor_group, int n_tensors) {
    if (n_tensors != t.n()) return fail(std::string(what) + ": tensor_group must hold one entry per parameter tensor");
    for (int i = 0; i < n_tensors; ++i)
        if (tensor_group[i] < -1 || tensor_group[i] >= M2F_ADAM_MAX_GROUPS) return fail(std::string(what) + ": group index out of range");
    return 0;
}

namespace {
// The tensors of `group` (one entry per tensor, < 0: left out; null: every tensor) cut into slices of at most M2F_PARAM_SLICE elements;
// tag = the tensor's group, or its index without a map.  Pads between tensors are in no slice.  begin[j] = first slice of the j-th
// tensor that was cut, one more entry = their number.
void cut_slices(const ParamTable& t, const int* group, std::vector<ParamSlice>& out, std::vector<int>& begin) {
    for (int i = 0; i < t.n(); ++i) {
        if (group && group[i] < 0) continue;
        begin.push_back((int)out.size());
        for (int64_t e = 0; e < t.numels[i]; e += M2F_PARAM_SLICE) {
            ParamSlice sl;
            sl.off = t.offsets[i] + e; sl.n = (int)std::min<int64_t>(M2F_PARAM_SLICE, t.numels[i] - e); sl.tag = group ? group[i] : i;
            out.push_back(sl);
        }
    }
    begin.push_back((int)out.size());
}

// Parameters [first, end) of the flat buffers = the run [i0, i1) of whole tensors: `first` is the offset of a tensor; end < 0, or beyond
// the last tensor's offset: to the end; otherwise the offset of a tensor behind `first`.  `what`: the entry point's name for messages.
int tensor_range(const char* what, const ParamTable& t, int64_t first, int64_t end, int* i0, int* i1) {
    const int n = t.n();
    const auto at = [&](int64_t off) { return (int)(std::lower_bound(t.offsets.begin(), t.offsets.end(), off) - t.offsets.begin()); };
    *i0 = at(first);
    *i1 = end >= 0 ? std::max(*i0, at(end)) : n;
    if (*i0 >= n || t.offsets[*i0] != first || *i1 <= *i0)
        return fail(std::string(what) + ": [first, end) must start at a parameter tensor and hold at least one");
    if (end >= 0 && *i1 < n && t.offsets[*i1] != end)
        return fail(std::string(what) + ": `end` must be the offset of a parameter tensor (or < 0)");
    return 0;
}

// A table in device memory.  ALL_SLICES: every tensor's slices (tag = tensor index) with the first slice of every tensor behind them -
// what the norm and the statistics walk; kept for the life of the process.  OWNED_ITEMS / OWNED_SLICES: the tensors some group of `map`
// owns, as the grouped kernels walk them - items re-tiled from 0 with their groups (shadow-writing form) or slices tagged with the group
// (flat form, exchange).  An optimizer has one map until add_param_group changes it, so those stay few: beyond 32 the oldest goes
// (after a device sync: a kernel may read it).  SAM_ITEMS: every tensor's item, 1-D runs cut at the tensor's last element (the host
// table's run on to the next tensor: its pad is the Adam kernel's to rewrite, nobody else's), re-tiled from 0 - what the shadow-writing
// perturbation walks; no map, kept for the life of the process.
enum TableKind { ALL_SLICES, OWNED_ITEMS, OWNED_SLICES, SAM_ITEMS };
struct DeviceTable {
    const ParamTable* host = nullptr; int device = -1; TableKind kind = ALL_SLICES; std::vector<int> map;      // the key
    std::vector<int> own_before;             // [n + 1]: owned tensors in front of tensor i
    std::vector<int> begin;                  // first tile / slice of owned tensor j; [n_owned] = their number
    void* dev = nullptr;
    const AdamItem* items = nullptr; const int* tb = nullptr; const int* grp = nullptr;
    const ParamSlice* slices = nullptr; const int* slice_begin = nullptr;
    int count() const { return begin.back(); }
};
std::vector<DeviceTable*> g_device_tables;

// `what`: the entry point's name for messages; map: null for ALL_SLICES, else one checked entry per tensor (group_map_bad)
const DeviceTable* device_table(const char* what, const ParamTable& host, TableKind kind, const int* map) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { fail(std::string(what) + ": no current device"); return nullptr; }
    const size_t n = (size_t)host.n(), nm = map ? n : 0;
    std::lock_guard<std::mutex> lock(g_mu);
    for (const DeviceTable* t : g_device_tables)
        if (t->host == &host && t->device == device && t->kind == kind && t->map.size() == nm &&
            (!nm || memcmp(t->map.data(), map, sizeof(int) * nm) == 0))
            return t;
    std::unique_ptr<DeviceTable> t(new DeviceTable);
    t->host = &host; t->device = device; t->kind = kind; t->map.assign(map, map + nm);
    int owned = 0;
    for (size_t i = 0; i < n; ++i) { t->own_before.push_back(owned); owned += !map || map[i] >= 0; }
    t->own_before.push_back(owned);
    std::vector<char*> d;
    if (kind == SAM_ITEMS) {
        std::vector<AdamItem> items = host.items;
        for (size_t i = 0; i < n; ++i)
            if (items[i].rows == 0) items[i].cols = (int)host.numels[i];
        retile(items, nullptr, false, t->begin);
        if (upload_packed(t->dev, {{items.data(), items.size() * sizeof(AdamItem)}, {t->begin.data(), t->begin.size() * sizeof(int)}}, d))
            return nullptr;
        t->items = reinterpret_cast<const AdamItem*>(d[0]); t->tb = reinterpret_cast<const int*>(d[1]);
    } else if (kind == OWNED_ITEMS) {
        std::vector<AdamItem> items = host.items;
        std::vector<int> grp = t->map;
        retile(items, &grp, false, t->begin);
        if (owned) {
            if (upload_packed(t->dev, {{items.data(), items.size() * sizeof(AdamItem)}, {t->begin.data(), t->begin.size() * sizeof(int)},
                                       {grp.data(), grp.size() * sizeof(int)}}, d)) return nullptr;
            t->items = reinterpret_cast<const AdamItem*>(d[0]); t->tb = reinterpret_cast<const int*>(d[1]); t->grp = reinterpret_cast<const int*>(d[2]);
        }
    } else {
        std::vector<ParamSlice> slices;
        cut_slices(host, map, slices, t->begin);
        if (owned) {
            if (upload_packed(t->dev, {{slices.data(), slices.size() * sizeof(ParamSlice)}, {t->begin.data(), t->begin.size() * sizeof(int)}}, d))
                return nullptr;
            t->slices = reinterpret_cast<const ParamSlice*>(d[0]); t->slice_begin = reinterpret_cast<const int*>(d[1]);
        }
    }
    if (map) {
        size_t mapped = 0;
        for (const DeviceTable* x : g_device_tables) mapped += !x->map.empty();
        if (mapped >= 32) {
            auto oldest = std::find_if(g_device_tables.begin(), g_device_tables.end(), [](const DeviceTable* x) { return !x->map.empty(); });
            (void)hipDeviceSynchronize();
            if ((*oldest)->dev) (void)hipFree((*oldest)->dev);
            delete *oldest;
            g_device_tables.erase(oldest);
        }
    }
    g_device_tables.push_back(t.release());
    return g_device_tables.back();
}

int tstats_bins_bad(const char* what, int bins) {
    if (bins < 2 || bins > M2F_TSTATS_MAX_BINS)
        return fail(std::string(what) + ": bins must be in [2, " + std::to_string(M2F_TSTATS_MAX_BINS) + "] (got " + std::to_string(bins) + ")");
    return 0;
}
}  // namespace
}  // namespace m2f

using namespace m2f;

extern "C" {

// ---- parameter shadows shared by the plans of one model + the optimizer that keeps them current -------------------------
int64_t m2f_param_shadow_elems(const m2f_config* cfg) {
    const ParamTable* t = param_table(*cfg, true);
    return t ? (int64_t)t->shadow_elems + ADAM_TABLE_BYTES / 2 : -1;
}

int m2f_param_shadow_init(const m2f_config* cfg, uint16_t* param_shadow, m2f_stream_t stream) {
    const ParamTable* t = param_table(*cfg, true);
    if (!t) return 1;
    if (!param_shadow || (reinterpret_cast<uintptr_t>(param_shadow) & 255)) return fail("m2f_param_shadow_init: 256-byte aligned buffer required");
    hipStream_t s = static_cast<hipStream_t>(stream);
    M2F_HIP(hipMemsetAsync(param_shadow, 0, t->shadow_elems * sizeof(uint16_t) + ADAM_TABLE_BYTES, s));      // the pad columns of the shadows stay zero for good
    char* tab = reinterpret_cast<char*>(param_shadow + t->shadow_elems);
    M2F_HIP(hipMemcpyAsync(tab, t->items.data(), t->items.size() * sizeof(AdamItem), hipMemcpyHostToDevice, s));
    M2F_HIP(hipMemcpyAsync(tab + t->items.size() * sizeof(AdamItem), t->tile_begin.data(), t->tile_begin.size() * sizeof(int), hipMemcpyHostToDevice, s));
    M2F_HIP(hipStreamSynchronize(s));
    return 0;
}

// `what`: the entry point's name for messages; ema == NULL: without the average stream
static int adam_step_shadowed_range(const char* what, const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg,
                                    float* exp_avg_sq, uint16_t* param_shadow, float* ema, float ema_w, int64_t first, int64_t end, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                                    m2f_stream_t stream) {
    const ParamTable* t = param_table(*cfg, true);
    if (!t) return 1;
    int i0, i1;
    if (tensor_range(what, *t, first, end, &i0, &i1)) return 1;
    const char* tab = reinterpret_cast<const char*>(param_shadow + t->shadow_elems);
    const AdamItem* items = reinterpret_cast<const AdamItem*>(tab);
    const int* tile_begin = reinterpret_cast<const int*>(tab + t->items.size() * sizeof(AdamItem));
    M2F_HIP(m2f_launch_adam_shadowed(params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, items + i0, tile_begin + i0, i1 - i0,
                                     t->tile_begin[i0], t->tile_begin[i1], lr, beta1, beta2, eps, weight_decay, step,
                                     grad_scale_ptr, ema, ema_w, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adam_step_shadowed_range(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg,
                                 float* exp_avg_sq, uint16_t* param_shadow, int64_t first, int64_t end, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int step, const float* grad_scale_ptr, m2f_stream_t stream) {
    return adam_step_shadowed_range("m2f_adam_step_shadowed_range", cfg, params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, nullptr,
                                    0.f, first, end, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr, stream);
}

int m2f_adam_step_shadowed_range_ema(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg,
                                     float* exp_avg_sq, uint16_t* param_shadow, float* ema, float ema_w, int64_t first, int64_t end,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                     const float* grad_scale_ptr, m2f_stream_t stream) {
    if (ema_args_bad("m2f_adam_step_shadowed_range_ema", ema, ema_w)) return 1;
    return adam_step_shadowed_range("m2f_adam_step_shadowed_range_ema", cfg, params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, ema,
                                    ema_w, first, end, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr, stream);
}

int m2f_adam_step_shadowed(const m2f_config* cfg, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           uint16_t* param_shadow, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           const float* grad_scale_ptr, m2f_stream_t stream) {
    return m2f_adam_step_shadowed_range(cfg, params, grads, 0, exp_avg, exp_avg_sq, param_shadow, 0, -1, lr, beta1, beta2, eps,
                                        weight_decay, step, grad_scale_ptr, stream);
}

// ---- parameter groups (m2f_adam_hyper_groups / m2f_adam_step_grouped) ---------------------------------------------------------------
int m2f_adam_hyper_groups(float* hyper_table, const m2f_adam_group* groups, int n_groups, m2f_stream_t stream) {
    if (!hyper_table || !groups) return fail("m2f_adam_hyper_groups: NULL buffer");
    if (n_groups < 1 || n_groups > M2F_ADAM_MAX_GROUPS) return fail("m2f_adam_hyper_groups: 1 .. 16 groups");
    float rows[M2F_ADAM_MAX_GROUPS * 8];
    for (int i = 0; i < n_groups; ++i) {
        const m2f_adam_group& g = groups[i];
        if (g.step < 1) return fail("m2f_adam_hyper_groups: step < 1");
        // lr / bc1 and 1 / sqrt(bc2) exactly as m2f_launch_adam forms them (lr arrives there as a float)
        const double bc1 = 1.0 - pow((double)g.beta1, g.step), bc2 = 1.0 - pow((double)g.beta2, g.step);
        float* r = rows + 8 * i;
        r[0] = (float)((double)(float)g.lr / bc1); r[1] = g.beta1; r[2] = g.beta2; r[3] = g.eps;
        r[4] = g.decoupled ? 0.f : g.weight_decay;
        r[5] = (float)(1.0 / sqrt(bc2));
        r[6] = g.decoupled ? (float)(1.0 - g.lr * (double)g.weight_decay) : 1.0f;
        r[7] = 0.f;
    }
    M2F_HIP(m2f_launch_adam_hyper_groups(hyper_table, rows, n_groups, static_cast<hipStream_t>(stream)));
    return 0;
}

static int adam_step_grouped(const char* what, const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg, float* exp_avg_sq,
                             uint16_t* param_shadow, float* ema, float ema_w, const int* tensor_group, int n_tensors, const float* hyper_table,
                             int64_t first, int64_t end, const float* grad_scale_ptr, m2f_stream_t stream) {
    if (!cfg || !params || !grads || !exp_avg || !exp_avg_sq || !tensor_group || !hyper_table) return fail(std::string(what) + ": NULL configuration / buffer");
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) return fail(std::string(what) + ": the flat buffers must be 16-byte aligned");
    const ParamTable* h = param_table(*cfg, param_shadow != nullptr);
    if (!h || group_map_bad(what, *h, tensor_group, n_tensors)) return 1;
    int i0, i1;
    if (tensor_range(what, *h, first, end, &i0, &i1)) return 1;
    const DeviceTable* t = device_table(what, *h, param_shadow ? OWNED_ITEMS : OWNED_SLICES, tensor_group);
    if (!t) return 1;
    const int j0 = t->own_before[i0], j1 = t->own_before[i1];        // of the range's tensors, the owned ones
    if (j1 <= j0) return 0;                                  // no group owns a tensor of the range: nothing to do
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (param_shadow)
        M2F_HIP(m2f_launch_adam_shadowed_grouped(params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, t->items + j0, t->tb + j0,
                                                 t->grp + j0, j1 - j0, t->begin[j0], t->begin[j1], hyper_table, grad_scale_ptr, ema, ema_w, s));
    else
        M2F_HIP(m2f_launch_adam_slices(params, grads, grads_bf16, exp_avg, exp_avg_sq, t->slices, t->begin[j0], t->begin[j1], hyper_table,
                                       grad_scale_ptr, ema, ema_w, s));
    return 0;
}

int m2f_adam_step_grouped(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg, float* exp_avg_sq,
                          uint16_t* param_shadow, const int* tensor_group, int n_tensors, const float* hyper_table, int64_t first,
                          int64_t end, const float* grad_scale_ptr, m2f_stream_t stream) {
    return adam_step_grouped("m2f_adam_step_grouped", cfg, params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, nullptr, 0.f, tensor_group, n_tensors,
                             hyper_table, first, end, grad_scale_ptr, stream);
}

int m2f_adam_step_grouped_ema(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg, float* exp_avg_sq,
                              uint16_t* param_shadow, float* ema, float ema_w, const int* tensor_group, int n_tensors,
                              const float* hyper_table, int64_t first, int64_t end, const float* grad_scale_ptr, m2f_stream_t stream) {
    if (ema_args_bad("m2f_adam_step_grouped_ema", ema, ema_w)) return 1;
    return adam_step_grouped("m2f_adam_step_grouped_ema", cfg, params, grads, grads_bf16, exp_avg, exp_avg_sq, param_shadow, ema, ema_w, tensor_group, n_tensors,
                             hyper_table, first, end, grad_scale_ptr, stream);
}

int m2f_ema_exchange(const m2f_config* cfg, float* params, float* ema, const int* tensor_group, int n_tensors, m2f_stream_t stream) {
    if (!cfg || !params || !ema || !tensor_group) return fail("m2f_ema_exchange: NULL configuration / buffer");
    if (params == ema) return fail("m2f_ema_exchange: params and ema are the same buffer");
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(ema)) & 15) return fail("m2f_ema_exchange: the flat buffers must be 16-byte aligned");
    const ParamTable* h = param_table(*cfg);
    if (!h || group_map_bad("m2f_ema_exchange", *h, tensor_group, n_tensors)) return 1;
    const DeviceTable* t = device_table("m2f_ema_exchange", *h, OWNED_SLICES, tensor_group);      // the slice list of the owned tensors
    if (!t) return 1;
    if (!t->count()) return 0;
    M2F_HIP(m2f_launch_ema_exchange(params, ema, t->slices, 0, t->count(), static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- global gradient norm and the clip record (gradnorm.hip) ---------------------------------------------------------------------
int64_t m2f_grad_norm_scratch_bytes(const m2f_config* cfg) {
    if (!cfg) { fail("m2f_grad_norm_scratch_bytes: NULL configuration"); return -1; }
    const ParamTable* h = param_table(*cfg);
    return h ? (int64_t)std::max(h->slice_begin.back(), 1) * (int64_t)sizeof(double) : -1;
}

int m2f_grad_sumsq(const m2f_config* cfg, const void* grads, int grads_bf16, int64_t first, int64_t end, double* scratch, int grid,
                   int nontemporal, m2f_stream_t stream) {
    if (!cfg || !grads || !scratch) return fail("m2f_grad_sumsq: NULL configuration / buffer");
    if (reinterpret_cast<uintptr_t>(grads) & 15) return fail("m2f_grad_sumsq: the gradient buffer must be 16-byte aligned");
    const ParamTable* h = param_table(*cfg);
    int i0, i1;
    if (!h || tensor_range("m2f_grad_sumsq", *h, first, end, &i0, &i1)) return 1;
    const DeviceTable* t = device_table("m2f_grad_norm", *h, ALL_SLICES, nullptr);
    if (!t) return 1;
    M2F_HIP(m2f_launch_grad_sumsq(grads, grads_bf16, t->slices, h->slice_begin[i0], h->slice_begin[i1], scratch, grid, nontemporal,
                                  static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_grad_norm_finalize(const m2f_config* cfg, const double* scratch, const float* den_ptr, double max_norm, float* record,
                           m2f_stream_t stream) {
    if (!cfg || !scratch || !record) return fail("m2f_grad_norm_finalize: NULL configuration / buffer");
    if (!(max_norm > 0.0)) return fail("m2f_grad_norm_finalize: max_norm must be positive");
    const ParamTable* h = param_table(*cfg);
    if (!h) return 1;
    M2F_HIP(m2f_launch_grad_norm_finalize(scratch, h->slice_begin.back(), den_ptr, max_norm, record, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- sharpness-aware minimisation (sam.hip) --------------------------------------------------------------------------------------
int m2f_sam_perturb(const m2f_config* cfg, float* params, const float* grads, const uint16_t* grads_bf16, float* saved, uint16_t* param_shadow,
                    const double* scratch, const float* grad_scale_ptr, double rho, float* record, m2f_stream_t stream) {
    if (!cfg || !params || !saved || !scratch || !record) return fail("m2f_sam_perturb: NULL configuration / buffer");
    if (!grads == !grads_bf16) return fail("m2f_sam_perturb: exactly one of grads / grads_bf16");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail("m2f_sam_perturb: rho must be a finite number > 0");
    const void* g = grads ? static_cast<const void*>(grads) : static_cast<const void*>(grads_bf16);
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(saved)) & 15)
        return fail("m2f_sam_perturb: the flat buffers must be 16-byte aligned");
    if (params == saved) return fail("m2f_sam_perturb: params and saved are the same buffer");
    if (param_shadow && (reinterpret_cast<uintptr_t>(param_shadow) & 255)) return fail("m2f_sam_perturb: 256-byte aligned shadow buffer required");
    const ParamTable* h = param_table(*cfg, param_shadow != nullptr);
    if (!h) return 1;
    const DeviceTable* t = device_table("m2f_sam_perturb", *h, param_shadow ? SAM_ITEMS : ALL_SLICES, nullptr);
    if (!t) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    M2F_HIP(m2f_launch_sam_finalize(scratch, h->slice_begin.back(), grad_scale_ptr, rho, record, s));
    if (param_shadow)
        M2F_HIP(m2f_launch_sam_perturb_shadowed(params, g, grads_bf16 != nullptr, saved, param_shadow, t->items, t->tb, h->n(), t->count(), record, s));
    else
        M2F_HIP(m2f_launch_sam_perturb_flat(params, g, grads_bf16 != nullptr, saved, t->slices, h->slice_begin.back(), record, s));
    return 0;
}

int m2f_sam_restore(const m2f_config* cfg, float* params, const float* saved, m2f_stream_t stream) {
    if (!cfg || !params || !saved) return fail("m2f_sam_restore: NULL configuration / buffer");
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(saved)) & 15) return fail("m2f_sam_restore: the flat buffers must be 16-byte aligned");
    if (params == saved) return fail("m2f_sam_restore: params and saved are the same buffer");
    const ParamTable* h = param_table(*cfg);
    if (!h) return 1;
    const DeviceTable* t = device_table("m2f_sam_restore", *h, ALL_SLICES, nullptr);
    if (!t) return 1;
    M2F_HIP(m2f_launch_sam_restore(params, saved, t->slices, h->slice_begin.back(), static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- per-tensor statistics and histograms (tensor_stats.hip) -----------------------------------------------------------------------
int64_t m2f_tensor_stats_scratch_bytes(const m2f_config* cfg, int bins) {
    if (!cfg) { fail("m2f_tensor_stats_scratch_bytes: NULL configuration"); return -1; }
    if (tstats_bins_bad("m2f_tensor_stats_scratch_bytes", bins)) return -1;
    const ParamTable* h = param_table(*cfg);
    return h ? (int64_t)std::max(h->slice_begin.back(), 1) * (int64_t)sizeof(StatPartial) : -1;
}

int64_t m2f_tensor_stats_record_bytes(const m2f_config* cfg, int bins) {
    if (!cfg) { fail("m2f_tensor_stats_record_bytes: NULL configuration"); return -1; }
    if (tstats_bins_bad("m2f_tensor_stats_record_bytes", bins)) return -1;
    const ParamTable* h = param_table(*cfg);
    return h ? 8 * ((int64_t)M2F_TSTATS_HEADER + (int64_t)h->n() * (M2F_TSTATS_FIELDS + bins)) : -1;
}

int m2f_tensor_stats_passes(const m2f_config* cfg, const void* a, int a_is_bf16, const float* b, int bins, const float* den_ptr, void* scratch,
                            void* record, int grid, int nontemporal, int passes, m2f_stream_t stream) {
    if (!cfg || !a || !scratch || !record) return fail("m2f_tensor_stats: NULL configuration / buffer");
    if (tstats_bins_bad("m2f_tensor_stats", bins)) return 1;
    if (a_is_bf16 && b) return fail("m2f_tensor_stats: the difference form a - b takes fp32 buffers only");
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) return fail("m2f_tensor_stats: the flat buffers must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(scratch) | reinterpret_cast<uintptr_t>(record)) & 7) return fail("m2f_tensor_stats: scratch and record must be 8-byte aligned");
    if (passes < 1 || passes > 3) return fail("m2f_tensor_stats: passes must be 1, 2 or 3");
    const ParamTable* h = param_table(*cfg);
    const DeviceTable* t = h ? device_table("m2f_tensor_stats", *h, ALL_SLICES, nullptr) : nullptr;
    if (!t) return 1;
    M2F_HIP(m2f_launch_tensor_stats(a, a_is_bf16, b, t->slices, t->slice_begin, t->count(), h->n(), bins, den_ptr,
                                    static_cast<StatPartial*>(scratch), static_cast<double*>(record), grid, nontemporal, passes,
                                    static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_tensor_stats(const m2f_config* cfg, const void* a, int a_is_bf16, const float* b, int bins, const float* den_ptr, void* scratch,
                     void* record, int grid, int nontemporal, m2f_stream_t stream) {
    return m2f_tensor_stats_passes(cfg, a, a_is_bf16, b, bins, den_ptr, scratch, record, grid, nontemporal, 3, stream);
}

}  // extern "C"
