// The plan object behind the C ABI (include/m2fnet_hip.h) and what its translation units share: plan_build.hip builds the launch lists,
// plan.hip runs them (executor, graph cache, switches), plan_stream.hip holds the stream / chunk plans, entry_kernels.hip the kernel-level
// entry points.  Internal: host code only, never installed, included by no kernel file.
#pragma once
#include "../../include/m2fnet_hip.h"
#include "common.h"
#include "ops.h"
#include "param_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

struct m2f_plan;
namespace m2f __attribute__((visibility("hidden"))) {      // (this part of the namespace is not part of the library's surface)

// ---------------------------------------------------------------------------------------------------
// ops, launches
// ---------------------------------------------------------------------------------------------------
enum OpKind { OP_GEMM, OP_ATTN_FWD, OP_ATTN_BWD, OP_LN_FWD, OP_LN_BWD, OP_DROPOUT };

struct Op {
    int kind = OP_GEMM;
    int layout = M2F_LAYOUT_NT;
    std::vector<GemmProblem> gp;
    std::vector<AttnProblem> ap;
    std::vector<LnProblem> lp;
    float* dptr = nullptr; int dT = 0, dd = 0, dld = 0; uint32_t dsite = 0;      // OP_DROPOUT
    std::vector<std::pair<int, int>> src;       // (chain id, index in that chain) of the ops merged into this one
    int group = 0;                              // 0 modality encoders + projections, 1 fusion stack (reference src/model.py:13-20,129-131), 2 classifier
};

struct Launch {
    int kind = OP_GEMM;
    int layout = M2F_LAYOUT_NT;
    GemmBatch gb;
    AttnBatch ab;
    AttnStreamBatch sb;                               // stream plans (m2f_plan_create_stream): what an OP_ATTN_FWD launch runs instead of `ab`
    AttnStreamWeights sw{}; bool sw_on = false;       // ... and, with m2f_plan_stream_attention on, where each of its problems stores its rows of probabilities
    LnBatch lb;
    float* dptr = nullptr; int dT = 0, dd = 0, dld = 0; uint32_t dsite = 0;
    float* dptr2 = nullptr; uint32_t dsite2 = 0;      // OP_DROPOUT: a second buffer of the same shape in the same launch
    std::vector<std::pair<int, int>> src;
    int group = 0;
};

struct Arena {
    char* base = nullptr;
    size_t off = 0;
    template <typename T> T* alloc(size_t n) {
        off = (off + 255) / 256 * 256;
        T* p = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
    float* f(size_t n) { return alloc<float>(n); }
};

inline GemmProblem gp_make(const float* a, int lda, const float* b, int ldb, int M, int N, int K, float* c, int ldc) {
    GemmProblem p;
    memset(&p, 0, sizeof(p));
    p.a.p[0] = a; p.a.ld[0] = lda; p.a.k[0] = K;
    p.b.p[0] = b; p.b.ld[0] = ldb; p.b.k[0] = K;
    p.M = M; p.N = N; p.c = c; p.ldc = ldc; p.gate_scale = 1.f;
    return p;
}
inline void gp_seg2(GemmProblem& p, const float* a1, int lda1, const float* b1, int ldb1, int K1) {
    p.a.p[1] = a1; p.a.ld[1] = lda1; p.a.k[1] = K1;
    p.b.p[1] = b1; p.b.ld[1] = ldb1; p.b.k[1] = K1;
}

struct EncLayerBuf {
    const float* y_in; float *qkv, *probs, *att, *s1, *st1, *y1, *h, *s2, *st2, *y2;
    uint32_t site_attn, site_d1, site_ff, site_d2;
};
struct ModBuf {
    int d = 0, H = 0, nl = 0, nt = 0;
    const float* x_in = nullptr;
    std::vector<std::vector<EncLayerBuf>> L;
    std::vector<float*> xe, stf;
    float* xp = nullptr;
    uint32_t site_pre = 0, site_post = 0;
};
struct FamBuf { const float* t_in; float *qv, *k, *probs, *att, *x, *t_out; uint32_t site_attn, site_out; };

// Which part of the backward a call runs: all of it (m2f_backward, m2f_step), or part 0 / 1 of the split step (m2f_step_part; see
// Built::bwd_head).
enum BwdPart { BWD_WHOLE = -1, BWD_HEAD = 0, BWD_TAIL = 1 };
// The form of a call's weight gradients (wg_form in plan.hip decides it, once): the table launch's instantiation and the tail that follows
// it.  The split step always writes fp32 gradients: its parts run the plain table launch over their own tile lists, whatever is armed.
enum WgForm { WG_PLAIN = 0, WG_ACCUMULATE, WG_GRAD_BF16, WG_ADAM, WG_ADAM_GROUPED, WG_SPLIT_PART };

// What a captured step depends on beyond the launch lists: the step's arguments, the switches that choose launches, and the
// plan's generation (bumped whenever a pointer or table that captured launches hold is replaced).
struct GraphKey {
    float ls; int cw, norm, fresh, form; uint64_t gen; const void* record;       // form: a WgForm; record: the one m2f_eval_step's launches add to
    bool operator==(const GraphKey& o) const {
        return ls == o.ls && cw == o.cw && norm == o.norm && fresh == o.fresh && form == o.form && gen == o.gen && record == o.record;
    }
    // the key of a capture without a backward (stream step, chunk call; eval step: its criterion arguments and its record)
    static GraphKey forward(bool fresh, uint64_t gen, float ls = 0.f, int cw = 0, const void* record = nullptr) {
        return {ls, cw, 0, (int)fresh, WG_PLAIN, gen, record};
    }
};
struct GraphSlot { hipGraphExec_t exec = nullptr; GraphKey key{}; void reset() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; } };
// (SLOT_STEP_ACC: the step in the accumulate form, m2f_plan_accumulate_grads - its own slot, so that a plan alternating between the two
//  forms replays both graphs instead of capturing one again at every switch)
// (SLOT_EVAL: forward + scoring, m2f_eval_step - the one slot eval plans use)
// (SLOT_STREAM: the step of a stream plan, m2f_stream_step)
// (SLOT_PREFILL: the chunk call of a chunk plan, m2f_stream_prefill)
enum { SLOT_STEP = 0, SLOT_PART0, SLOT_PART1, SLOT_STEP_ACC, SLOT_EVAL, SLOT_STREAM, SLOT_PREFILL, SLOT_COUNT };

// An attention site of the plan in state_dict order (m2f_plan_attention_sites): kind 0 = audio_encoders.{a}.layers.{b}.self_attn, 1 = text_encoders.{a}.layers.{b}.self_attn,
// 2 = fusion_layers.{a}.multihead_attention; probs: the P^T its forward saves (m2f_plan_attention_weights reads it)
struct AttnSiteRef { int kind, a, b, H, hd; const float* probs; };

// Everything build_plan and its helpers write.  A rebuild is `built = Built{}` followed by build_plan: a field added here cannot survive one.
struct Built {
    // bf16 mode: shadows of the workspace activations (same element index) and of the 2-D parameters (padded rows)
    ShadowMap sh = {nullptr, nullptr, 0};
    uint16_t* wshadow = nullptr;
    std::vector<CastBatch> param_casts;  // bf16 mode, at the start of a forward: every 2-D parameter -> its W and W^T shadows ...
    std::vector<CastBatch> input_casts;  // ... and the two input staging buffers -> their activation shadows
    std::vector<Launch> fwd, bwd;
    std::vector<AttnSiteRef> attn_sites;
    // deferred weight-gradient launches, run after the backward chain on the same stream.  (Overlapping them with the
    // chain on a second stream was measured SLOWER inside the captured graph: every fork costs the chain a 12-16 us
    // cross-queue gap and the chain's small GEMMs run ~2x longer next to a chip-filling launch; 2.85 -> 2.77 ms/step.)
    std::vector<Launch> wg;
    std::vector<Launch> wg_rest;     // weight gradients the table launch cannot take
    std::vector<CastBatch> wg_casts;  // ... and the narrow operands it takes as padded bf16 copies made in front of it
    // bf16 mode: all weight gradients as ONE persistent GEMM launch over a device-resident problem table, on the row-major
    // bf16 shadows of dY / X (the launch also sums the bias gradients); wg_table: it runs instead of wg's grouped launches
    bool wg_table = false;
    GemmBatch wg_tab{};
    std::vector<GemmProblem> tprobs_host;        // the table's problems as uploaded (host copy)
    double wg_flops = 0.0;
    // SPLIT backward (m2f_step_part; data-parallel overlap): part 0 = forward + criterion + the classifier / fusion-stack backward
    // chain (bwd[0, bwd_head)) + the weight gradients whose operands that chain completes; part 1 = the encoders' backward +
    // the rest.  The fusion stack's and the classifier's gradients are the TAIL of the flat buffer (from split_offset on): their
    // all-reduce can travel under part 1.  Same table, two tile lists.
    size_t bwd_head = 0;
    bool split_ok = false;
    int64_t split_offset = 0;
    GemmBatch wg_tab_part[2] = {};
    size_t wg_rest_head = 0;             // wg_rest[0, wg_rest_head) belong to part 0
    int n_no_f32 = 0;                    // outputs whose fp32 copy is not written (mark_unread_fp32)
    std::vector<LnReduceBatch> lnred;
    size_t ws_used = 0;
};

// A form of the weight-gradient table launch that a switch arms (m2f_plan_fused_adam_setup, m2f_plan_grad_bf16): the table launch with the
// form's own problem table, and the items of the ONE launch behind the backward that handles what the table does not cover (1-D
// parameters, weight gradients of wg_rest).  Both read from one device blob.
struct TableForm {
    GemmBatch tab{};
    void* dev = nullptr;                 // one hipMalloc (upload_packed): [M2FAdamFuse |] GemmProblem[] | AdamItem[] | int tile_begin[] [| int group[]]
    const AdamItem* items = nullptr; const int* tile_begin = nullptr; int n_items = 0, tiles = 0;
    bool ready = false, on = false;
    void disarm() { ready = on = false; }        // a rebuild: the uploaded problems point into the old lists' operands - set up again
    TableForm() = default; TableForm(const TableForm&) = delete;
    ~TableForm() { if (dev) (void)hipFree(dev); }
};
// ... and what only the optimizer form holds (gemm_p8.h EPI 3): the optimizer's buffers, its step-dependent factors in device memory so
// that the captured graph stays valid from step to step; grouped (m2f_plan_fused_adam_setup_grouped): EPI 6, the problems carry their
// group's hyper row, the residual launch is the grouped shadow-writing kernel over the owned tensors (grp parallel to items; none left: no launch)
struct FusedBufs {
    float *p = nullptr, *m = nullptr, *v = nullptr; uint16_t* sh = nullptr; const float *hyper = nullptr, *gs = nullptr;
    bool grouped = false; const int* grp = nullptr;
};
// ACCUMULATE form (m2f_plan_accumulate_grads): every launch that writes a parameter gradient or the criterion tail adds to what the
// buffer holds (old + new, one rounded fp32 add).  The table launch and the LayerNorm reduces take the same arguments in their
// accumulate instantiations; the grouped weight-gradient launches are copies of wg / wg_rest with GF_ACCUM, built on first use.
struct AccForm {
    bool on = false, ready = false;
    std::vector<Launch> wg, wg_rest;
    void disarm() { ready = false; wg.clear(); wg_rest.clear(); }      // (`on` stays: the lists follow a rebuild, build_accumulate)
};

// The criterion's state (m2f_plan_distill, m2f_plan_focal, m2f_plan_rdrop, m2f_plan_crf, m2f_plan_supcon, m2f_plan_aux_head): which form
// do_loss launches.  The switches exclude each other by plan.hip's exclusions[] table (focal combines with distillation and with the
// auxiliary head; nothing else does).
struct Criterion {
    bool distill_on = false;             // the teacher blend (M2F_BUF_TEACHER, alpha and tau = M2F_BUF_DISTILL)
    bool focal_on = false;               // do_loss and the eval rows launch run their focal forms (gamma = M2F_BUF_FOCAL[0])
    bool rdrop_on = false;               // the R-Drop criterion (twins = M2F_BUF_PARTNER, alpha = M2F_BUF_RDROP[0])
    float* rdrop_kl = nullptr;           // ... its per-row KL terms [T] (train plans), reduced into the tail's fourth float
    // m2f_plan_supcon: do_loss runs the supervised contrastive kernels (supcon.hip) on the classifier's last hidden activation behind the
    // cross-entropy launch, the backward adds their gradient behind the GEMM that writes that activation's gradient (bwd[0]).  Train plans;
    // the buffers sit at the end of the workspace, (lambda, tau) = M2F_BUF_SUPCON
    bool supcon_on = false;
    float* supcon_ws = nullptr;          // m2f_supcon_ws_floats(T, cls_hidden) floats
    float* supcon_rows = nullptr;        // [T, 4] row terms (lse, n, l, w l); w l reduced into the tail's fourth float
    float* supcon_dfeat = nullptr;       // [T, pad8(cls_hidden)]: the unnormalised gradient w.r.t. the stored activation
    float* supcon_scale = nullptr;       // [1]: what the finalize launch multiplies dlogits by (1 / den, or 1)
    float* supcon_dh = nullptr;          // the chain's gradient of that activation (bwd[0]'s output) ...
    float supcon_gate = 1.f;             // ... and its gate scale (the dropout scale when the activation carries a dropout site)
    // m2f_plan_aux_head: do_loss runs the auxiliary label head's rows kernel (aux_head.hip) on the same activation behind the cross-entropy
    // launch, the backward joins its gradient behind bwd[0] (supcon_dh / supcon_gate: the same join point, so the two exclude each other)
    // and, with a trainable block, writes the block's gradient.  The block and its gradient are the CALLER's (never part of the flat
    // buffer); (lambda, eps_a) = M2F_BUF_AUX, the labels = M2F_BUF_AUX_LABELS, the logits = M2F_BUF_AUX_LOGITS
    bool aux_on = false;
    const float* aux_params = nullptr;   // [W (aux_A x cls_hidden) | b (aux_A)]
    float* aux_grad = nullptr;           // the same size, or null (frozen)
    int aux_A = 0;
    float* aux_ws = nullptr;             // m2f_aux_head_ws_floats(T, cls_hidden, 16) floats: g [T, 16] | row terms [T] | the gradient's partials
    float* aux_scale = nullptr;          // [1]: what the finalize launch multiplies dlogits by (1 / den, or 1)
    // m2f_plan_crf: do_loss runs the linear-chain CRF criterion (crf.hip), the eval step the CRF loss and the Viterbi path.  The parameter
    // block and its gradient are the CALLER's (never part of the flat buffer); crf_ws / crf_pred / crf_score sit at the end of the workspace
    bool crf_on = false;
    const float* crf_params = nullptr;   // [C*C + 2C] (stream and chunk plans: the block m2f_plan_stream_crf filters over)
    float* crf_grad = nullptr;           // [C*C + 2C] or null (frozen)
    float* crf_ws = nullptr;             // m2f_crf_scratch_floats(T, B, C) floats (null: a stream plan, or cls_out outside 2 .. 16)
    int32_t* crf_pred = nullptr;         // [T]
    float* crf_score = nullptr;          // [B]
};

// plan.hip
m2f_plan* plan_new(const m2f_config* cfg, int B, int L, int precision, int train, int T_packed = 0);
int do_forward(m2f_plan& P, hipStream_t s);
// Replays the graph of slot `g`, captured from `body` first - again whenever the slot's key differs from the call's.
int replay_slot(GraphSlot& g, const GraphKey& key, hipStream_t s, const std::function<int()>& body);
// The one size-then-build path.  `dry`: a fresh plan of the wanted kind and settings, no buffer bound (deleted here), built against a null workspace -
// `shared`: with a sentinel for parameter shadows outside the plan.  need = its size + slack.  P == null (the sizing queries): done.  Otherwise need is
// compared with P->ws_bytes, `before_build` runs, P->built is cleared and built in P->ws_base, and its size compared again.  Size failures: the caller words them.
enum BuildStatus { BUILD_OK = 0, BUILD_FAILED, BUILD_TOO_SMALL, BUILD_OVERRAN };
BuildStatus size_and_build(m2f_plan* dry, bool shared, int64_t slack, m2f_plan* P, int64_t& need, const std::function<int()>& before_build = nullptr);
// plan_build.hip
int build_plan(m2f_plan& P, char* ws_base);
void apply_speakers(m2f_plan& P);      // the plan's speaker-head setting into every attention launch of the built lists
int build_accumulate(m2f_plan& P);
extern "C" __attribute__((visibility("default")))      // (an accident of the library's symbol list, kept: internal, nothing outside the library may call it)
int table_coverage(m2f_plan& P, uint16_t* param_shadow, std::vector<GemmProblem>& tp, std::vector<int>& tensor_of, std::vector<AdamItem>& items, std::vector<int>& tensor);
}  // namespace m2f

struct m2f_plan {
    m2f_config cfg;
    int B = 0, L = 0, T = 0, prec = 0, train = 0;
    float* params = nullptr; float* grads = nullptr;
    char* ws_base = nullptr;         // the caller's workspace (m2f_plan_backward_outputs rebuilds the launch lists in it)
    int64_t ws_bytes = 0;
    // what the backward computes (m2f_plan_backward_outputs): d loss / d input of the modalities in `in_mask` (1 text, 2 audio) into
    // M2F_BUF_DTEXT / M2F_BUF_DAUDIO, and (param_grads) the parameter gradients.  Default (0, 1): parameter gradients only.
    int in_mask = 0, param_grads = 1;
    int band_past = -1, band_future = -1;   // context band of every attention launch (m2f_plan_attention_band); negative = unlimited
    float bias_gain = 0.f;                  // distance-decay bias of every attention launch (m2f_plan_attention_bias): the applied gain, 0 = off
    // speaker heads of every attention launch (m2f_plan_attention_speakers): same-speaker / other-speaker heads per site, (0, 0) = off; the ids are
    // M2F_BUF_SPEAKERS.  Stream and chunk plans: s_spk = the caller's array of cached ids, uint8 [S][C] by logical row (m2f_plan_stream_speakers)
    int spk_same = 0, spk_other = 0;
    uint8_t* s_spk = nullptr;
    bool packed = false; int* cu = nullptr;      // T token rows owned by B dialogues through cu_seqlens, device int32 [B + 1] (m2f_plan_create_packed)
    // STREAM plan (m2f_plan_create_stream): B = S stream slots of L = 1 row each, forward only; every attention site runs the streaming
    // kernel (attention_stream.hip) against its own K / V caches of `s_cap` rows per slot, a ring when the context band has a window
    bool streaming = false;
    int s_cap = 0, s_ring = 0;
    int* s_len = nullptr;            // device int32 [S]: utterances cached per slot (M2F_BUF_STREAM_LEN)
    uint8_t* s_active = nullptr;     // device uint8 [S]: slots that take an utterance in the next step (M2F_BUF_STREAM_ACTIVE)
    int64_t s_cache_bytes = 0;
    // PAGED stream plan (m2f_plan_create_stream_paged): the sites hold page pools instead of per-slot caches, s_pg.table (M2F_BUF_STREAM_TABLE)
    // maps a slot's logical rows to pages; one table for every site.  A chunk plan copies its parent's paging.
    int s_pages = 0;                 // pages of every pool (0: dense caches)
    AttnStreamPaging s_pg = {nullptr, 0, 0, 0, 0};
    // CHUNK plan (m2f_plan_create_stream_chunk): B = S slots of L = s_chunk rows each over the caches and counters of `s_parent`, a stream
    // plan of the same configuration; every attention site runs the chunk kernel (attention_stream_chunk.hip).  It owns no cache.
    m2f_plan* s_parent = nullptr; int s_chunk = 0;
    int* s_new = nullptr;            // device int32 [S]: utterances each slot takes in the next m2f_stream_prefill (M2F_BUF_STREAM_NEW)
    float* s_attn = nullptr;         // m2f_plan_stream_attention: the caller's [sites][S][H][C] buffer the step's attention launches fill (M2F_BUF_STREAM_ATTN; null: off)
    uint32_t* rng = nullptr; bool use_dropout = false;
    uint32_t drop_thresh = 0; float drop_scale = 1.f;
    m2f::ParamMap pm;
    void* bufs[M2F_BUF_LIMIT] = {nullptr};
    float* loss_terms = nullptr;
    int* eval_partial = nullptr;     // m2f_eval_step: the rows launch's integer tiles (its row terms go to loss_terms, as the criterion's do)
    bool eval_warmed = false;        // ... and one eager m2f_eval_step before its first capture (`warmed` belongs to the train step)
    // The parameter shadows may live OUTSIDE the plan (m2f_plan_create_shared: one buffer shared by all plans of a model) and be
    // kept current by the optimizer itself (m2f_adam_step_shadowed); the caller then declares them fresh
    // (m2f_plan_params_fresh) and the forward skips the parameter casts.
    uint16_t* ext_wshadow = nullptr;
    bool params_fresh = false;
    m2f::Built built;                // the launch lists and what goes with them (build_plan)
    // What the switches arm.  Optimizer in the weight-gradient launch's epilogue (m2f_plan_fused_adam_setup / m2f_plan_fused_adam): the table launch in
    // its Adam form + ONE launch of the shadow-writing Adam kernel over the rest.  Gradients left as bf16 (m2f_plan_grad_bf16): the table launch writes
    // dW as bf16 into `g16_buf` (same element index as the fp32 buffer), one cast launch at the end of the backward rounds every other gradient into it.
    m2f::TableForm fused, g16;
    m2f::FusedBufs fz;
    uint16_t* g16_buf = nullptr;
    m2f::AccForm acc;
    m2f::Criterion crit;             // which criterion do_loss launches, and what it needs
    // m2f_plan_adversarial: the modalities that hold a perturbation, and per modality (0 text, 1 audio) delta and x_clean inside the caller's
    // state buffer; hyper / skip / scratch are bufs[M2F_BUF_ADV], bufs[M2F_BUF_ADV_SKIP] and adv_scratch
    int adv_mask = 0;
    float* adv_delta[2] = {nullptr, nullptr}; float* adv_clean[2] = {nullptr, nullptr};
    double* adv_scratch = nullptr;
    float* s_phi = nullptr;              // stream and chunk plans (m2f_plan_stream_crf): the CALLER's filter state [S, C] over crf_params, or null
    // graph cache: m2f_step, m2f_step_part(0), m2f_step_part(1), ...
    m2f::GraphSlot graphs[m2f::SLOT_COUNT];
    uint64_t generation = 0;      // bumped by every entry point that replaces what captured launches point to (invalidate in plan.hip)
    bool warmed = false;          // one eager step (sets kernel attributes) before the first capture
    ~m2f_plan() { for (m2f::GraphSlot& g : graphs) g.reset(); }
};
