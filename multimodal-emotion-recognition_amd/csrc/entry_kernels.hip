// Entry points of the C ABI (include/m2fnet_hip.h) that never touch a plan: the gather, RNG and optimizer steps, and the kernel-level
// test and encoder entry points (m2f_gemm, m2f_attention_*, m2f_layernorm_*, m2f_w2v_*, m2f_mel_*) with their thread-local shadow map.
#include "plan.h"

using namespace m2f;

extern "C" {

int m2f_gather_dialogues(const float* text_table, int d_text, const float* audio_table, int d_audio,
                         const int64_t* label_table, const int32_t* rows, int T, float* text_out, int ld_text,
                         float* audio_out, int ld_audio, uint8_t* key_pad_out, int64_t* labels_out, m2f_stream_t stream) {
    GatherArgs a;
    a.text_table = text_table; a.audio_table = audio_table; a.label_table = label_table; a.rows = rows;
    a.T = T; a.d_text = d_text; a.d_audio = d_audio; a.ld_text = ld_text; a.ld_audio = ld_audio;
    a.text_out = text_out; a.audio_out = audio_out; a.key_pad = key_pad_out; a.labels = labels_out;
    M2F_HIP(m2f_launch_gather(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_rng_advance(uint32_t* rng_state, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_rng_advance(rng_state, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_adam(params, grads, 0, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr,
                            nullptr, 0.f, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adam_step_g16(float* params, const uint16_t* grads_bf16, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale_ptr,
                      m2f_stream_t stream) {
    M2F_HIP(m2f_launch_adam(params, grads_bf16, 1, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr,
                            nullptr, 0.f, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int step, float ema_w, const float* grad_scale_ptr, m2f_stream_t stream) {
    if (ema_args_bad("m2f_adam_step_ema", ema, ema_w)) return 1;
    M2F_HIP(m2f_launch_adam(params, grads, 0, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr, ema, ema_w,
                            static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adam_step_g16_ema(float* params, const uint16_t* grads_bf16, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float ema_w, const float* grad_scale_ptr,
                          m2f_stream_t stream) {
    if (ema_args_bad("m2f_adam_step_g16_ema", ema, ema_w)) return 1;
    M2F_HIP(m2f_launch_adam(params, grads_bf16, 1, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_ptr,
                            ema, ema_w, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- kernel-level entry points -----------------------------------------------------------------------
// Optional bf16 shadow map for the kernel-level entry points (the plans carry their own): outputs that lie inside
// [ws_base, ws_base + floats) are also written as bf16 at the same element index of `shadow`.
static thread_local ShadowMap g_sh = {nullptr, nullptr, 0};
int m2f_set_shadow_map(const float* ws_base, uint16_t* shadow, int64_t floats) {
    if ((ws_base == nullptr) != (shadow == nullptr) || floats < 0) return fail("m2f_set_shadow_map: base / shadow must both be set or both be NULL");
    g_sh = {ws_base, shadow, (size_t)floats};
    return 0;
}

static thread_local int g_shadow_only = 0;
int m2f_set_shadow_only(int on) { g_shadow_only = on != 0; return 0; }

static void drop_params(float p, uint32_t* thresh, float* scale) {
    *thresh = (uint32_t)std::min(4294967295.0, std::floor((double)p * 4294967296.0));
    *scale = 1.0f / (1.0f - p);
}

int m2f_gemm(int precision, int layout, int M, int N, int K0, int K1, const float* a0, int lda0, const float* a1, int lda1,
             const float* b0, int ldb0, const float* b1, int ldb1, float* c, int ldc, const float* bias, const float* res,
             int ldres, const float* gate, int ldgate, float gate_scale, float* bias_grad, int relu_a, int relu_b,
             int relu_out, int accumulate, uint32_t drop_site, float drop_p, const uint32_t* rng_state, int tile,
             float* splitk_ws, uint32_t* splitk_tickets, int splitk_max_tiles,
             const uint16_t* a0q, int ldaq0, const uint16_t* a1q, int ldaq1,
             const uint16_t* b0q, int ldbq0, const uint16_t* b1q, int ldbq1, m2f_stream_t stream) {
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    GemmProblem p = gp_make(a0, lda0, b0, ldb0, M, N, K0, c, ldc);
    if (K1 > 0) gp_seg2(p, a1, lda1, b1, ldb1, K1);
    p.bias = bias; p.res = res; p.ldres = ldres; p.gate = gate; p.ldgate = ldgate; p.gate_scale = gate_scale;
    p.bias_grad = bias_grad; p.drop_site = drop_site;
    p.flags = (relu_a ? GF_RELU_A : 0) | (relu_b ? GF_RELU_B : 0) | (relu_out == 1 ? GF_RELU_OUT : 0) |
              (relu_out == 2 ? GF_GELU_OUT : 0) | (accumulate ? GF_ACCUM : 0) | (g_shadow_only && !accumulate ? GF_NO_F32 : 0);
    p.a.q[0] = a0q; p.a.ldq[0] = ldaq0; p.a.q[1] = a1q; p.a.ldq[1] = ldaq1;
    p.b.q[0] = b0q; p.b.ldq[0] = ldbq0; p.b.q[1] = b1q; p.b.ldq[1] = ldbq1;
    p.a.qt[0] = p.a.qt[1] = p.b.qt[0] = p.b.qt[1] = nullptr;
    gb.pr[0] = p; gb.count = 1; gb.rng = rng_state; gb.sh = g_sh;
    gb.splitk_ws = splitk_ws; gb.splitk_cnt = splitk_tickets; gb.splitk_max_tiles = splitk_ws && splitk_tickets ? splitk_max_tiles : 0;
    if (drop_site) drop_params(drop_p, &gb.drop_thresh, &gb.drop_scale);
    M2F_HIP(m2f_launch_gemm(gb, precision, layout, tile, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_quantize_fp8(const float* src, uint8_t* dst, int64_t n, float scale, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_quant_fp8(src, dst, n, scale, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_gemm_fp8(int M, int N, int K, const uint8_t* a8, int lda, const uint8_t* b8, int ldb, float acc_scale, float* c, int ldc,
                 const float* bias, const float* res, int ldres, int activation, uint8_t* c8, float c8_scale,
                 m2f_stream_t stream) {
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    GemmProblem p;
    memset(&p, 0, sizeof(p));
    p.a.q[0] = reinterpret_cast<const uint16_t*>(a8); p.a.ldq[0] = lda; p.a.k[0] = K;
    p.b.q[0] = reinterpret_cast<const uint16_t*>(b8); p.b.ldq[0] = ldb; p.b.k[0] = K;
    p.M = M; p.N = N; p.c = c; p.ldc = ldc; p.bias = bias; p.res = res; p.ldres = ldres;
    p.gate_scale = 1.f; p.acc_scale = acc_scale; p.c8 = c8; p.c8_scale = c8_scale;
    if (!c && !c8) return fail("m2f_gemm_fp8: no output buffer");
    p.flags = (activation == 1 ? GF_RELU_OUT : 0) | (activation == 2 ? GF_GELU_OUT : 0) | (g_shadow_only && c && !c8 ? GF_NO_F32 : 0);
    gb.pr[0] = p; gb.count = 1; gb.sh = g_sh;
    M2F_HIP(m2f_launch_gemm_fp8(gb, static_cast<hipStream_t>(stream)));
    return 0;
}

static void attn_fill(AttnBatch& ab, int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                      const float* v, int ldv, const uint8_t* key_pad, float* out, int ldo, float* probs, uint32_t drop_site,
                      float drop_p, const uint32_t* rng_state) {
    memset(&ab, 0, sizeof(ab));
    AttnProblem& p = ab.pr[0];
    p.q = q; p.k = k; p.v = v; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.out = out; p.ldo = ldo; p.probs = probs;
    p.H = H; p.hd = hd; p.drop_site = drop_site;
    ab.count = 1; ab.B = B; ab.L = L; ab.key_pad = key_pad; ab.rng = rng_state;
    ab.drop_scale = 1.f;
    ab.sh = g_sh;                                              // (m2f_set_shadow_map: operands / results inside that range have bf16 copies)
    {   // kernel-level tests of the bf16-mode forms: M2F_ATTN_BF16_KERNEL=<mask> (AttnBatch::bf16_math), read per call
        const char* e = getenv("M2F_ATTN_BF16_KERNEL");
        ab.bf16_math = e ? atoi(e) & 63 : 0;
    }
    if (drop_site) drop_params(drop_p, &ab.drop_thresh, &ab.drop_scale);
}

/* a gain option -> what the launch descriptor holds: finite, >= 0, rounded to bf16 */
static int bias_gain_ok(const char* who, float gain, float* applied) {
    if (!(gain >= 0.f) || !std::isfinite(gain)) return fail(std::string(who) + ": gain must be finite and >= 0");
    *applied = m2f_attn_bias_gain(m2f_attn_bias_gain16(gain));
    if (!std::isfinite(*applied)) return fail(std::string(who) + ": gain is out of range");
    return 0;
}
/* the speaker-head counts: >= 0, together at most H, and ids wherever a count is non-zero */
static int speaker_heads_ok(const char* who, int H, int n_same, int n_other, const void* ids, const char* what) {
    const std::string w(who);
    if (n_same < 0 || n_other < 0) return fail(w + ": n_same and n_other must be >= 0");
    if (n_same > 255 || n_other > 255 || n_same + n_other > H)
        return fail(w + ": n_same + n_other = " + std::to_string(n_same + n_other) + " exceeds the " + std::to_string(H) + " heads");
    if ((n_same | n_other) && !ids) return fail(w + ": speaker heads need " + what);
    return 0;
}
/* m2f_attn_opts -> the launch descriptor of a forward entry (NULL: no option); every refusal comes before the launch */
static int attn_apply(const char* who, AttnBatch& ab, const m2f_attn_opts* opts) {
    static const m2f_attn_opts none = M2F_ATTN_OPTS_NONE;
    const m2f_attn_opts& o = opts ? *opts : none;
    float g = 0.f;
    if (int r = bias_gain_ok(who, o.bias_gain, &g)) return r;
    if (int r = speaker_heads_ok(who, ab.pr[0].H, o.n_same, o.n_other, o.speakers, "speakers (uint8, one per token row)")) return r;
    m2f_attn_set_band(ab, o.past, o.future);
    ab.bias_gain16 = m2f_attn_bias_gain16(g);
    ab.speaker = (o.n_same | o.n_other) ? o.speakers : nullptr; ab.spk_same = (uint8_t)o.n_same; ab.spk_other = (uint8_t)o.n_other;
    return 0;
}
static void attn_bwd_fill(AttnBatch& ab, const float* dout, int lddo, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                          int past, int future) {
    AttnProblem& p = ab.pr[0];
    p.dout = dout; p.lddo = lddo; p.dq = dq; p.dk = dk; p.dv = dv; p.lddq = lddq; p.lddk = lddk; p.lddv = lddv;
    m2f_attn_set_band(ab, past, future);               // (short: the saved P^T carries the band; long: the block pairs the forward skipped)
}
int m2f_attention_fwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                      const uint8_t* key_pad, float* out, int ldo, float* probs, uint32_t drop_site, float drop_p,
                      const uint32_t* rng_state, m2f_stream_t stream, const m2f_attn_opts* opts) {
    AttnBatch ab;
    attn_fill(ab, B, L, H, hd, q, ldq, k, ldk, v, ldv, key_pad, out, ldo, probs, drop_site, drop_p, rng_state);
    if (int r = attn_apply("m2f_attention_fwd", ab, opts)) return r;
    M2F_HIP(m2f_launch_attn_fwd(ab, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_attention_bwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                      const uint8_t* key_pad, const float* out, int ldo, const float* probs, const float* dout, int lddo,
                      float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, uint32_t drop_site, float drop_p,
                      const uint32_t* rng_state, m2f_stream_t stream, int past, int future) {
    AttnBatch ab;
    attn_fill(ab, B, L, H, hd, q, ldq, k, ldk, v, ldv, key_pad, const_cast<float*>(out), ldo, const_cast<float*>(probs),
              drop_site, drop_p, rng_state);
    attn_bwd_fill(ab, dout, lddo, dq, lddq, dk, lddk, dv, lddv, past, future);
    M2F_HIP(m2f_launch_attn_bwd(ab, static_cast<hipStream_t>(stream)));
    return 0;
}

static int attn_varlen_fill(const char* who, AttnBatch& ab, int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                            const float* v, int ldv, const int32_t* cu, int T, const uint8_t* key_pad, float* out, int ldo, float* probs,
                            uint32_t drop_site, float drop_p, const uint32_t* rng_state) {
    const std::string w(who);
    if (B < 1 || L < 1 || L > M2F_ATTN_DLONG_MAX_L) return fail(w + ": 1 <= L <= 512 required (got L = " + std::to_string(L) + ")");
    if (!cu == !key_pad) return fail(w + ": exactly one of cu (packed rows) and key_pad (padded rows) must be given");
    if (cu && T < 1) return fail(w + ": packed rows need T >= 1");
    if (!m2f_attn_dlong_index_ok(B, H, L)) return fail(w + ": B * H * L * L must stay below 2^32");
    attn_fill(ab, B, L, H, hd, q, ldq, k, ldk, v, ldv, key_pad, out, ldo, probs, drop_site, drop_p, rng_state);
    ab.bf16_math = 0;                                          // (the long-dialogue kernels read fp32 operands only)
    ab.cu = cu; ab.T = cu ? T : B * L;
    return 0;
}
int m2f_attention_varlen_fwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                             const int32_t* cu, int T, const uint8_t* key_pad, float* out, int ldo, float* probs, uint32_t drop_site,
                             float drop_p, const uint32_t* rng_state, m2f_stream_t stream, const m2f_attn_opts* opts) {
    AttnBatch ab;
    if (attn_varlen_fill("m2f_attention_varlen_fwd", ab, B, L, H, hd, q, ldq, k, ldk, v, ldv, cu, T, key_pad, out, ldo, probs, drop_site, drop_p, rng_state)) return -1;
    if (int r = attn_apply("m2f_attention_varlen_fwd", ab, opts)) return r;
    M2F_HIP(m2f_launch_attn_dlong_fwd(ab, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_attention_varlen_bwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                             const int32_t* cu, int T, const uint8_t* key_pad, const float* out, int ldo, const float* probs,
                             const float* dout, int lddo, float* dq, int lddq, float* dk, int lddk, float* dv, int lddv,
                             uint32_t drop_site, float drop_p, const uint32_t* rng_state, m2f_stream_t stream, int past, int future) {
    AttnBatch ab;
    if (attn_varlen_fill("m2f_attention_varlen_bwd", ab, B, L, H, hd, q, ldq, k, ldk, v, ldv, cu, T, key_pad, const_cast<float*>(out), ldo, const_cast<float*>(probs),
                         drop_site, drop_p, rng_state)) return -1;
    attn_bwd_fill(ab, dout, lddo, dq, lddq, dk, lddk, dv, lddv, past, future);
    M2F_HIP(m2f_launch_attn_dlong_bwd(ab, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_attention_stream_cache_elems(int S, int H, int hd, int C, int bf16) {
    if (S < 1 || H < 1 || hd < 1 || hd > 128 || C < 1 || C > M2F_ATTN_STREAM_MAX_C) { fail("m2f_attention_stream_cache_elems: S, H >= 1, 1 <= hd <= 128, 1 <= C <= 512 required"); return -1; }
    return (int64_t)m2f_attn_stream_cache_elems(S, H, hd, C, bf16 != 0);
}
int64_t m2f_attention_stream_pool_elems(int n_pages, int H, int hd, int R, int bf16) {
    if (n_pages < 1 || H < 1 || hd < 1 || hd > 128 || (R != 16 && R != 32 && R != 64)) { fail("m2f_attention_stream_pool_elems: n_pages, H >= 1, 1 <= hd <= 128, R in {16, 32, 64} required"); return -1; }
    return (int64_t)m2f_attn_stream_pool_elems(n_pages, H, hd, R, bf16 != 0);
}
static int paged_args_ok(const char* who, int S, int H, int hd, int C, int n_pages, int R, int table_cols, const void* kpool, const void* vpool, const void* table) {
    const std::string w(who);
    if (S < 1 || H < 1 || hd < 1 || hd > 128 || C < 1 || C > M2F_ATTN_STREAM_MAX_C) return fail(w + ": S, H >= 1, 1 <= hd <= 128, 1 <= C <= 512 required");
    if (R != 16 && R != 32 && R != 64) return fail(w + ": page_rows must be 16, 32 or 64");
    if (n_pages < 1) return fail(w + ": n_pages >= 1 required");
    if (!kpool || !vpool || !table) return fail(w + ": NULL argument");
    if (table_cols != (C + R - 1) / R) return fail(w + ": the table must be int32 [S, ceil(C / page_rows)]");
    if ((reinterpret_cast<uintptr_t>(kpool) & 15) || (reinterpret_cast<uintptr_t>(vpool) & 15)) return fail(w + ": the pools must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(table) & 3) return fail(w + ": the table must be 4-byte aligned");
    return 0;
}
/* The two kernel-level launches: one argument check and one batch fill.  chunk: the chunk form of T rows per slot (`second` = n_new),
   otherwise the step form (`second` = active); a table in the options: kc / vc are the pools, otherwise dense caches. */
static int stream_attn_fill(const char* who, AttnStreamBatch& sb, const m2f_attn_stream_opts* o, int S, bool chunk, int T, int H, int hd, const float* q, int ldq,
                            const float* k, int ldk, const float* v, int ldv, void* kc, void* vc, int C, int ring, const int32_t* count,
                            const void* second, float* out, int ldo, int bf16) {
    const std::string w(who);
    const bool t_ok = !chunk || (T >= 1 && T <= M2F_ATTN_STREAM_MAX_CHUNK), pg = o && o->table;
    if (pg) {
        if (int r = paged_args_ok(who, S, H, hd, C, o->n_pages, o->page_rows, o->table_cols, kc, vc, o->table)) return r;
        if (!t_ok) return fail(w + ": 1 <= T <= 64 required");
    } else if (S < 1 || H < 1 || hd < 1 || hd > 128 || C < 1 || C > M2F_ATTN_STREAM_MAX_C || !t_ok) {
        return fail(w + ": S, H >= 1, 1 <= hd <= 128, 1 <= C <= 512" + (chunk ? ", 1 <= T <= 64" : "") + " required");
    }
    if (!q || !k || !v || !kc || !vc || !count || !second || !out) return fail(w + ": NULL argument");
    if (ldq < H * hd || ldk < H * hd || ldv < H * hd || ldo < H * hd) return fail(w + ": a leading dimension is narrower than H * hd");
    if (!pg && ((reinterpret_cast<uintptr_t>(kc) & 15) || (reinterpret_cast<uintptr_t>(vc) & 15))) return fail(w + ": the caches must be 16-byte aligned");
    memset(&sb, 0, sizeof(sb));
    sb.count = 1; sb.S = S; sb.C = C; sb.ring = ring != 0; sb.bf16 = bf16 != 0; sb.len = count;
    sb.active = chunk ? nullptr : static_cast<const uint8_t*>(second);
    sb.sh = g_sh;
    AttnStreamProblem& p = sb.pr[0];
    p.q = q; p.k = k; p.v = v; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.out = out; p.ldo = ldo; p.kcache = kc; p.vcache = vc; p.H = H; p.hd = hd;
    return 0;
}
/* m2f_attn_stream_opts -> the batch, plus what a launcher takes beside it (NULL: no option); every refusal comes before the launch.
   chunk: spk_new holds T ids per slot, and there is no weights-emitting kernel */
struct StreamExtras {
    AttnStreamPaging pg;
    AttnStreamWeights ww;
    const AttnStreamPaging* paging = nullptr;
    const AttnStreamWeights* weights = nullptr;
};
static int stream_attn_apply(const char* who, AttnStreamBatch& sb, bool chunk, const m2f_attn_stream_opts* o, StreamExtras& x) {
    if (!o) return 0;
    const std::string w(who);
    float g = 0.f;
    if (int r = bias_gain_ok(who, o->bias_gain, &g)) return r;
    if (int r = speaker_heads_ok(who, sb.pr[0].H, o->n_same, o->n_other, o->spk_new,
                                 chunk ? "the new utterances' speakers (uint8 [S][T])" : "the new utterances' speakers (uint8 [S])")) return r;
    if ((o->n_same | o->n_other) && !o->spk_cache) return fail(w + ": speaker heads need the cached speakers (uint8 [S][C])");
    if (o->weights) {
        if (chunk) return fail(w + ": the chunk form emits no rows of probabilities, weights must be NULL");
        if (reinterpret_cast<uintptr_t>(o->weights) & 3) return fail(w + ": weights must be a 4-byte aligned device buffer of S * H * C floats");
        memset(&x.ww, 0, sizeof(x.ww));
        x.ww.w[0] = o->weights;
        x.weights = &x.ww;
    }
    if (o->table) { x.pg = {o->table, o->table_cols, o->page_rows, 0, o->n_pages}; x.paging = &x.pg; }
    sb.bias_gain = g;
    if (o->n_same | o->n_other) { sb.spk_cache = o->spk_cache; sb.spk_new = o->spk_new; sb.spk_same = (uint8_t)o->n_same; sb.spk_other = (uint8_t)o->n_other; }
    return 0;
}
int m2f_attention_stream(int S, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                         void* kcache, void* vcache, int C, int ring, const int32_t* count, const uint8_t* active, float* out, int ldo,
                         int bf16, m2f_stream_t stream, const m2f_attn_stream_opts* opts) {
    AttnStreamBatch sb;
    StreamExtras x;
    if (int r = stream_attn_fill("m2f_attention_stream", sb, opts, S, false, 1, H, hd, q, ldq, k, ldk, v, ldv, kcache, vcache, C, ring, count, active, out, ldo, bf16)) return r;
    if (int r = stream_attn_apply("m2f_attention_stream", sb, false, opts, x)) return r;
    M2F_HIP(m2f_launch_attn_stream(sb, x.paging, static_cast<hipStream_t>(stream), x.weights));
    return 0;
}
int m2f_attention_stream_chunk(int S, int T, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                               void* kcache, void* vcache, int C, int ring, const int32_t* count, const int32_t* n_new, float* out, int ldo,
                               int bf16, m2f_stream_t stream, const m2f_attn_stream_opts* opts) {
    AttnStreamBatch sb;
    StreamExtras x;
    if (int r = stream_attn_fill("m2f_attention_stream_chunk", sb, opts, S, true, T, H, hd, q, ldq, k, ldk, v, ldv, kcache, vcache, C, ring, count, n_new, out, ldo, bf16)) return r;
    if (int r = stream_attn_apply("m2f_attention_stream_chunk", sb, true, opts, x)) return r;
    M2F_HIP(m2f_launch_attn_stream_chunk(sb, x.paging, T, n_new, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_stream_advance_speakers(int S, int C, int ring, int32_t* count, const uint8_t* active, uint8_t* spk_cache, const uint8_t* spk_new,
                                m2f_stream_t stream) {
    if (S < 1 || C < 1 || C > M2F_ATTN_STREAM_MAX_C) return fail("m2f_stream_advance_speakers: S >= 1, 1 <= C <= 512 required");
    if (!count || !active || !spk_cache || !spk_new) return fail("m2f_stream_advance_speakers: NULL argument");
    M2F_HIP(m2f_launch_stream_advance_speakers(count, active, S, spk_cache, spk_new, C, ring != 0, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_stream_advance_speakers_n(int S, int T, int C, int ring, int32_t* count, const int32_t* n_new, uint8_t* spk_cache, const uint8_t* spk_new,
                                  m2f_stream_t stream) {
    if (S < 1 || C < 1 || C > M2F_ATTN_STREAM_MAX_C || T < 1 || T > M2F_ATTN_STREAM_MAX_CHUNK)
        return fail("m2f_stream_advance_speakers_n: S >= 1, 1 <= C <= 512, 1 <= T <= 64 required");
    if (!count || !n_new || !spk_cache || !spk_new) return fail("m2f_stream_advance_speakers_n: NULL argument");
    M2F_HIP(m2f_launch_stream_advance_speakers_n(count, n_new, S, T, spk_cache, spk_new, C, ring != 0, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_attention_speaker_class(int h, int n_same, int n_other) { return m2f_attn_speaker_class(h, n_same, n_other); }
int m2f_attention_opts_layout(int which, int* out, int max) {
    const std::vector<int> a = {(int)sizeof(m2f_attn_opts), (int)offsetof(m2f_attn_opts, past), (int)offsetof(m2f_attn_opts, future),
                                (int)offsetof(m2f_attn_opts, bias_gain), (int)offsetof(m2f_attn_opts, n_same), (int)offsetof(m2f_attn_opts, n_other),
                                (int)offsetof(m2f_attn_opts, speakers)};
    const std::vector<int> s = {(int)sizeof(m2f_attn_stream_opts), (int)offsetof(m2f_attn_stream_opts, table), (int)offsetof(m2f_attn_stream_opts, table_cols),
                                (int)offsetof(m2f_attn_stream_opts, n_pages), (int)offsetof(m2f_attn_stream_opts, page_rows),
                                (int)offsetof(m2f_attn_stream_opts, weights), (int)offsetof(m2f_attn_stream_opts, bias_gain),
                                (int)offsetof(m2f_attn_stream_opts, n_same), (int)offsetof(m2f_attn_stream_opts, n_other),
                                (int)offsetof(m2f_attn_stream_opts, spk_cache), (int)offsetof(m2f_attn_stream_opts, spk_new)};
    if (which != 0 && which != 1) { fail("m2f_attention_opts_layout: which must be 0 (m2f_attn_opts) or 1 (m2f_attn_stream_opts)"); return -1; }
    const std::vector<int>& v = which ? s : a;
    for (int i = 0; i < (int)v.size() && i < max && out; ++i) out[i] = v[i];
    return (int)v.size();
}

static int stream_cache_site(const char* who, int S, int H, int hd, void* kc, void* vc, const int32_t* table, int table_cols, int n_pages, int page_rows,
                             int C, int bf16, int n_entries, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets, void* packed,
                             int64_t packed_elems, int32_t* count, int scatter, m2f_stream_t stream) {
    const std::string w(who);
    const AttnStreamPaging paging = {table, table_cols, page_rows, 0, n_pages}, *pg = table ? &paging : nullptr;
    if (pg) {
        if (int r = paged_args_ok(who, S, H, hd, C, n_pages, page_rows, table_cols, kc, vc, table)) return r;
    } else {
        if (S < 1 || H < 1 || hd < 1 || hd > 128 || C < 1 || C > M2F_ATTN_STREAM_MAX_C) return fail(w + ": S, H >= 1, 1 <= hd <= 128, 1 <= C <= 512 required");
        if (!kc || !vc) return fail(w + ": NULL argument");
        if ((reinterpret_cast<uintptr_t>(kc) & 15) || (reinterpret_cast<uintptr_t>(vc) & 15)) return fail(w + ": the caches must be 16-byte aligned");
    }
    if (n_entries < 0 || packed_elems < 0) return fail(w + ": n_entries, packed_elems >= 0 required");
    if (!slots || !lengths || !row_offsets || !packed || (scatter && !count)) return fail(w + ": NULL argument");
    if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(w + ": the packed buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(row_offsets) & 7) return fail(w + ": row_offsets must be 8-byte aligned");
    StreamCacheBatch cb;
    memset(&cb, 0, sizeof(cb));
    const int vpr = m2f_stream_cache_row_vecs(hd, bf16 != 0);
    cb.count = 1;
    cb.site[0] = {kc, vc, H, vpr, 0, 0};
    cb.S = S; cb.C = C; cb.rowv = 2 * H * vpr; cb.n_entries = n_entries;
    cb.slots = slots; cb.lengths = lengths; cb.row_offsets = row_offsets;
    cb.packed = packed; cb.packed_vecs = packed_elems / (bf16 ? 8 : 4); cb.len = count;
    M2F_HIP(m2f_launch_stream_cache(cb, pg, scatter, static_cast<hipStream_t>(stream)));
    return 0;
}
int m2f_attention_stream_cache_gather(int S, int H, int hd, const void* kcache, const void* vcache, const int32_t* table, int table_cols,
                                      int n_pages, int page_rows, int C, int bf16, int n_entries, const int32_t* slots,
                                      const int32_t* lengths, const int64_t* row_offsets, void* packed, int64_t packed_elems,
                                      m2f_stream_t stream) {
    return stream_cache_site("m2f_attention_stream_cache_gather", S, H, hd, const_cast<void*>(kcache), const_cast<void*>(vcache), table, table_cols,
                             n_pages, page_rows, C, bf16, n_entries, slots, lengths, row_offsets, packed, packed_elems, nullptr, 0, stream);
}
int m2f_attention_stream_cache_scatter(int S, int H, int hd, void* kcache, void* vcache, const int32_t* table, int table_cols,
                                       int n_pages, int page_rows, int C, int bf16, int n_entries, const int32_t* slots,
                                       const int32_t* lengths, const int64_t* row_offsets, const void* packed, int64_t packed_elems,
                                       int32_t* count, m2f_stream_t stream) {
    return stream_cache_site("m2f_attention_stream_cache_scatter", S, H, hd, kcache, vcache, table, table_cols, n_pages, page_rows, C, bf16,
                             n_entries, slots, lengths, row_offsets, const_cast<void*>(packed), packed_elems, count, 1, stream);
}
int m2f_attention_weights(int B, int L, int H, const float* probs, const uint8_t* key_pad, const int32_t* cu, int past, int future,
                          int per_head, float* out, m2f_stream_t stream) {
    if (B < 1 || H < 1 || L < 1 || L > M2F_ATTN_DLONG_MAX_L) return fail("m2f_attention_weights: B, H >= 1 and 1 <= L <= 512 required");
    if (!probs || !out) return fail("m2f_attention_weights: NULL argument");
    if (cu && key_pad) return fail("m2f_attention_weights: at most one of cu (packed rows) and key_pad (padded rows) may be given");
    AttnWeightsBatch wb;
    memset(&wb, 0, sizeof(wb));
    wb.count = 1; wb.site[0] = {probs, out, H, 1.0f / (float)H};
    wb.B = B; wb.L = L; wb.per_head = per_head != 0; wb.key_pad = key_pad; wb.cu = cu;
    m2f_attn_weights_set_band(wb, past, future);
    M2F_HIP(m2f_launch_attn_weights(wb, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_attention_probs_elems(int B, int H, int L) { return (int64_t)m2f_attn_probs_elems(B, H, L); }

int m2f_layernorm_fwd(int T, int d, const float* x, const float* gamma, const float* beta, const float* res, float* out,
                      float* stats, float eps, m2f_stream_t stream) {
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    LnProblem& p = lb.pr[0];
    p.x = x; p.gamma = gamma; p.beta = beta; p.res = res; p.out = out; p.stats = stats; p.d = d;
    lb.count = 1; lb.T = T; lb.eps = eps; lb.drop_scale = 1.f; lb.sh = g_sh;
    M2F_HIP(m2f_launch_ln_fwd(lb, static_cast<hipStream_t>(stream)));
    return 0;
}

/* diagnostic (tools/ln_stats_ab.py; not in include/m2fnet_hip.h's product surface): the LayerNorm forward over `count` problems merged in one launch
 * as the plans do (x / out of problem i at x + i * T * ld ... the caller lays them out), statistics computed (pre = 0) or read from `stats` (pre = 1) */
int m2f_layernorm_fwd_diag(int T, int n_prob, const int* d, const float* const* x, const float* const* gamma, const float* const* beta, float* const* out,
                           float* const* stats, float eps, int pre, m2f_stream_t stream) {
    if (n_prob < 1 || n_prob > M2F_LN_MAX_PROBLEMS) return fail("m2f_layernorm_fwd_diag: 1..4 problems");
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    for (int i = 0; i < n_prob; ++i) {
        LnProblem& p = lb.pr[i];
        p.x = x[i]; p.gamma = gamma[i]; p.beta = beta[i]; p.out = out[i]; p.stats = stats[i]; p.d = d[i];
    }
    lb.count = n_prob; lb.T = T; lb.eps = eps; lb.drop_scale = 1.f; lb.sh = g_sh; lb.pre_stats = pre;
    M2F_HIP(m2f_launch_ln_fwd(lb, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_layernorm_fwd_out8(int T, int d, const float* x, const float* gamma, const float* beta, const float* res, float* out,
                           float* stats, float eps, uint8_t* out8, float out8_scale, m2f_stream_t stream) {
    if (!out8 || (d & 3) || (reinterpret_cast<uintptr_t>(out8) & 3)) return fail("m2f_layernorm_fwd_out8: e4m3 output needs d % 4 == 0 and a 4-byte aligned buffer");
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    LnProblem& p = lb.pr[0];
    p.x = x; p.gamma = gamma; p.beta = beta; p.res = res; p.out = out; p.stats = stats; p.d = d;
    lb.count = 1; lb.T = T; lb.eps = eps; lb.drop_scale = 1.f; lb.sh = g_sh; lb.out8 = out8; lb.out8_scale = out8_scale;
    M2F_HIP(m2f_launch_ln_fwd(lb, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_embed_layernorm(int T, int d, const int64_t* input_ids, const int64_t* position_ids, const float* word_emb,
                        const float* pos_emb, const float* type_emb_row0, const float* gamma, const float* beta, float eps,
                        float* out, int ld_out, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_embed_ln(input_ids, position_ids, word_emb, pos_emb, type_emb_row0, gamma, beta, eps, out, ld_out, T, d, g_sh,
                                static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_attention_long_fwd(int B, int S, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                           const uint8_t* key_pad, float* out, int ldo, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_attn_long_fwd(q, ldq, k, ldk, v, ldv, key_pad, out, ldo, B, S, H, hd, g_sh, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_attention_long_fwd_bf16(int B, int S, int H, int hd, const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v,
                                int ldv, const uint8_t* key_pad, uint16_t* out16, float* out32, int ldo, m2f_stream_t stream) {
    return m2f_attention_long_fwd_bf16_out8(B, S, H, hd, q, ldq, k, ldk, v, ldv, key_pad, out16, out32, nullptr, 1.f, ldo, stream);
}

int m2f_attention_long_fwd_bf16_out8(int B, int S, int H, int hd, const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v,
                                     int ldv, const uint8_t* key_pad, uint16_t* out16, float* out32, uint8_t* out8, float out8_scale, int ldo,
                                     m2f_stream_t stream) {
    if (!q || !k || !v || !(out16 || out32 || out8)) return fail("m2f_attention_long_fwd_bf16: NULL operand / no output");
    if (hd < 8 || hd > 128 || (hd & 7) || ((ldq | ldk | ldv | ldo) & 7))
        return fail("m2f_attention_long_fwd_bf16: head dim and leading dimensions must be multiples of 8, head dim <= 128");
    if (out8 && ((hd & 15) || (ldo & 15))) return fail("m2f_attention_long_fwd_bf16: the e4m3 output needs head dim and ldo in multiples of 16");
    M2F_HIP(m2f_launch_attn_long_fwd_bf16(q, ldq, k, ldk, v, ldv, key_pad, out16, out32, out8, out8_scale, ldo, B, S, H, hd, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_layernorm_bwd(int T, int d, const float* x, const float* gamma, const float* stats, const float* dy, const float* extra,
                      float* dx, float* partial, float* dgamma, float* dbeta, m2f_stream_t stream) {
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    LnProblem& p = lb.pr[0];
    p.x = x; p.gamma = gamma; p.stats = const_cast<float*>(stats); p.dy = dy; p.extra = extra; p.dx = dx; p.partial = partial; p.d = d;
    lb.count = 1; lb.T = T; lb.eps = 0.f; lb.drop_scale = 1.f;
    M2F_HIP(m2f_launch_ln_bwd(lb, static_cast<hipStream_t>(stream)));
    LnReduceBatch rb;
    memset(&rb, 0, sizeof(rb));
    rb.it[0].partial = partial; rb.it[0].dgamma = dgamma; rb.it[0].dbeta = dbeta; rb.it[0].d = d; rb.it[0].nblk = m2f_ln_row_blocks(T);
    rb.count = 1;
    M2F_HIP(m2f_launch_ln_param_reduce(rb, static_cast<hipStream_t>(stream)));
    return 0;
}

/* kernel-level tests of the dropout sites the row-wise kernels carry (tests/test_dropout_masks_gpu.py): the launches of the train plans */
int m2f_layernorm_fwd_drop(int T, int d, int ld, const float* x, const float* gamma, const float* beta, const float* res, float* out,
                           float* stats, float eps, uint32_t drop_site, float drop_p, const uint32_t* rng_state, m2f_stream_t stream) {
    if (ld && ld < d) return fail("m2f_layernorm_fwd_drop: ld must be 0 or at least d");
    if (drop_site && (!rng_state || !(drop_p > 0.f && drop_p < 1.f))) return fail("m2f_layernorm_fwd_drop: a site needs an rng_state and 0 < drop_p < 1");
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    LnProblem& p = lb.pr[0];
    p.x = x; p.gamma = gamma; p.beta = beta; p.res = res; p.out = out; p.stats = stats; p.d = d; p.ld = ld; p.drop_site = drop_site;
    lb.count = 1; lb.T = T; lb.eps = eps; lb.drop_scale = 1.f; lb.sh = g_sh; lb.rng = rng_state;
    if (drop_site) drop_params(drop_p, &lb.drop_thresh, &lb.drop_scale);
    M2F_HIP(m2f_launch_ln_fwd(lb, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_layernorm_bwd_masked(int T, int d, int ld, const float* x, const float* gamma, const float* stats, const float* dy,
                             const float* extra, float* dx, float* dx_masked, float* partial, float* dgamma, float* dbeta,
                             uint32_t drop_site2, float drop_p, const uint32_t* rng_state, m2f_stream_t stream) {
    if (ld && ld < d) return fail("m2f_layernorm_bwd_masked: ld must be 0 or at least d");
    if (drop_site2 && (!rng_state || !(drop_p > 0.f && drop_p < 1.f))) return fail("m2f_layernorm_bwd_masked: a site needs an rng_state and 0 < drop_p < 1");
    LnBatch lb;
    memset(&lb, 0, sizeof(lb));
    LnProblem& p = lb.pr[0];
    p.x = x; p.gamma = gamma; p.stats = const_cast<float*>(stats); p.dy = dy; p.extra = extra; p.dx = dx; p.dx_masked = dx_masked;
    p.partial = partial; p.d = d; p.ld = ld; p.drop_site2 = drop_site2;
    lb.count = 1; lb.T = T; lb.eps = 0.f; lb.drop_scale = 1.f; lb.rng = rng_state;
    if (drop_site2) drop_params(drop_p, &lb.drop_thresh, &lb.drop_scale);
    M2F_HIP(m2f_launch_ln_bwd(lb, static_cast<hipStream_t>(stream)));
    LnReduceBatch rb;
    memset(&rb, 0, sizeof(rb));
    rb.it[0].partial = partial; rb.it[0].dgamma = dgamma; rb.it[0].dbeta = dbeta; rb.it[0].d = d; rb.it[0].nblk = m2f_ln_row_blocks(T);
    rb.count = 1;
    M2F_HIP(m2f_launch_ln_param_reduce(rb, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_dropout_rows(float* x, float* x2, int T, int d, int ld, uint32_t site, uint32_t site2, float drop_p, const uint32_t* rng_state,
                     m2f_stream_t stream) {
    if (!x || !rng_state || T < 1 || d < 1 || ld < d) return fail("m2f_dropout_rows: NULL buffer / rng_state, or not 1 <= d <= ld");
    if (!(drop_p > 0.f && drop_p < 1.f)) return fail("m2f_dropout_rows: 0 < drop_p < 1 required");
    uint32_t thresh; float scale;
    drop_params(drop_p, &thresh, &scale);
    M2F_HIP(m2f_launch_dropout_inplace2(x, x2, T, d, ld, site, site2, rng_state, thresh, scale, g_sh, static_cast<hipStream_t>(stream)));
    return 0;
}

// The four m2f_cross_entropy* entries: their own checks and messages, then ONE filler (the common part of CeArgs) and ONE launch
// sequence (criterion, finalize, and the KL reduce where the criterion wrote KL terms).
static CeArgs ce_args(int T, int C, const float* logits, const int64_t* labels, const float* class_w, float label_smoothing,
                      float* loss_terms, float* dlogits) {
    CeArgs a;
    a.logits = logits; a.T = T; a.C = C; a.labels = labels; a.class_w = class_w; a.label_smoothing = label_smoothing;
    a.loss_terms = loss_terms; a.dlogits = dlogits;
    return a;
}

static int ce_run(const CeArgs& a, int normalise, float* loss_out, m2f_stream_t stream) {
    M2F_HIP(m2f_launch_ce(a, static_cast<hipStream_t>(stream)));
    M2F_HIP(m2f_launch_loss_finalize(a.loss_terms, a.T, a.C, a.dlogits, loss_out, normalise, static_cast<hipStream_t>(stream)));
    if (a.kl_terms) M2F_HIP(m2f_launch_rdrop_kl_reduce(a.kl_terms, a.T, loss_out, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_cross_entropy(int T, int C, const float* logits, const int64_t* labels, const float* class_w, float label_smoothing,
                      int normalise, float* loss_terms, float* dlogits, float* loss_out, m2f_stream_t stream) {
    return ce_run(ce_args(T, C, logits, labels, class_w, label_smoothing, loss_terms, dlogits), normalise, loss_out, stream);
}

int m2f_cross_entropy_distill(int T, int C, const float* logits, const float* teacher, const int64_t* labels, const float* class_w,
                              float label_smoothing, const float* hyper_dev, int normalise, float* loss_terms, float* dlogits,
                              float* loss_out, m2f_stream_t stream) {
    if (!logits || !teacher || !labels || !hyper_dev || !loss_terms || !dlogits || !loss_out)
        return fail("m2f_cross_entropy_distill: NULL logits / teacher / labels / hyper_dev / loss_terms / dlogits / loss_out");
    if (T < 1 || C < 1 || C > 16) return fail("m2f_cross_entropy_distill: T >= 1 and 1 <= C <= 16 required");
    CeArgs a = ce_args(T, C, logits, labels, class_w, label_smoothing, loss_terms, dlogits);
    a.teacher = teacher; a.hyper = hyper_dev;
    return ce_run(a, normalise, loss_out, stream);
}

int m2f_cross_entropy_focal(int T, int C, const float* logits, const float* teacher, const int64_t* labels, const float* class_w,
                            float label_smoothing, const float* hyper_dev, const float* gamma_dev, int normalise, float* loss_terms,
                            float* dlogits, float* loss_out, m2f_stream_t stream) {
    if (!logits || !labels || !gamma_dev || !loss_terms || !dlogits || !loss_out)
        return fail("m2f_cross_entropy_focal: NULL logits / labels / gamma_dev / loss_terms / dlogits / loss_out");
    if (teacher && !hyper_dev) return fail("m2f_cross_entropy_focal: a teacher needs hyper_dev (alpha, tau)");
    if (T < 1 || C < 1 || C > 16) return fail("m2f_cross_entropy_focal: T >= 1 and 1 <= C <= 16 required");
    CeArgs a = ce_args(T, C, logits, labels, class_w, label_smoothing, loss_terms, dlogits);
    a.teacher = teacher; a.hyper = teacher ? hyper_dev : nullptr; a.gamma = gamma_dev;
    return ce_run(a, normalise, loss_out, stream);
}

int m2f_cross_entropy_rdrop(int T, int C, const float* logits, const int32_t* partner, const int64_t* labels, const float* class_w,
                            float label_smoothing, const float* alpha_dev, int normalise, float* loss_terms, float* dlogits,
                            float* loss_out, m2f_stream_t stream) {
    if (!logits || !partner || !labels || !alpha_dev || !loss_terms || !dlogits || !loss_out)
        return fail("m2f_cross_entropy_rdrop: NULL logits / partner / labels / alpha_dev / loss_terms / dlogits / loss_out");
    if (T < 1 || C < 1 || C > 16) return fail("m2f_cross_entropy_rdrop: T >= 1 and 1 <= C <= 16 required");
    CeArgs a = ce_args(T, C, logits, labels, class_w, label_smoothing, loss_terms, dlogits);
    a.partner = partner; a.alpha = alpha_dev; a.kl_terms = loss_terms + (size_t)T * 2;
    return ce_run(a, normalise, loss_out, stream);
}

int64_t m2f_crf_scratch_floats(int T, int B, int C) {
    return T < 1 || B < 1 || C < 2 || C > 16 ? 0 : (int64_t)T * (2 * C + 2) + (int64_t)B * (C * C + 2 * C);
}

static int crf_shape_bad(const char* who, int T, int C, int B, int L, const int32_t* cu_seqlens) {
    if (T < 1 || B < 1 || C < 2 || C > 16) return fail(std::string(who) + ": T >= 1, B >= 1 and 2 <= C <= 16 required");
    if (!cu_seqlens && (L < 1 || (int64_t)B * L > T)) return fail(std::string(who) + ": without cu_seqlens, L >= 1 and B * L <= T required");
    return 0;
}

int m2f_crf_nll(int T, int C, int B, int L, const int32_t* cu_seqlens, const float* logits, const int64_t* labels, const float* params,
                int normalise, float* scratch, float* loss_terms, float* dlogits, float* param_grad, float* loss_out,
                m2f_stream_t stream) {
    if (!logits || !labels || !params || !scratch || !loss_terms || !loss_out)
        return fail("m2f_crf_nll: NULL logits / labels / params / scratch / loss_terms / loss_out");
    if (!dlogits && param_grad) return fail("m2f_crf_nll: param_grad needs dlogits (the parameter gradient comes out of the backward sweep)");
    if (crf_shape_bad("m2f_crf_nll", T, C, B, L, cu_seqlens)) return 1;
    CrfArgs a;
    a.logits = logits; a.T = T; a.C = C; a.labels = labels; a.params = params; a.cu_seqlens = cu_seqlens; a.B = B; a.L = L;
    a.ws = scratch; a.loss_terms = loss_terms; a.dlogits = dlogits;
    a.partial = param_grad ? scratch + (size_t)T * (2 * C + 2) : nullptr;
    M2F_HIP(m2f_launch_crf_nll(a, static_cast<hipStream_t>(stream)));
    // (dlogits NULL: the loss alone - nothing for the finalize launch to scale)
    M2F_HIP(m2f_launch_loss_finalize(loss_terms, T, C, dlogits, loss_out, dlogits ? normalise : 0, static_cast<hipStream_t>(stream)));
    if (param_grad) M2F_HIP(m2f_launch_crf_grad_reduce(a.partial, B, C, loss_out, normalise, param_grad, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_crf_viterbi(int T, int C, int B, int L, const int32_t* cu_seqlens, const float* logits, const uint8_t* mask, const float* params,
                    void* scratch, int32_t* pred, float* score, m2f_stream_t stream) {
    if (!logits || !mask || !params || !scratch || !pred || !score)
        return fail("m2f_crf_viterbi: NULL logits / mask / params / scratch / pred / score");
    if (crf_shape_bad("m2f_crf_viterbi", T, C, B, L, cu_seqlens)) return 1;
    CrfViterbiArgs a;
    a.logits = logits; a.T = T; a.C = C; a.mask = mask; a.params = params; a.cu_seqlens = cu_seqlens; a.B = B; a.L = L;
    a.ws = static_cast<int*>(scratch); a.pred = pred; a.score = score;
    M2F_HIP(m2f_launch_crf_viterbi(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_crf_filter(int S, int C, int rows, const float* logits, const float* params, const int32_t* count, const uint8_t* active,
                   const int32_t* n_new, float* phi, m2f_stream_t stream) {
    if (!logits || !params || !count || !phi) return fail("m2f_crf_filter: NULL logits / params / count / phi");
    if (S < 1 || rows < 1 || C < 2 || C > 16) return fail("m2f_crf_filter: S >= 1, rows >= 1 and 2 <= C <= 16 required");
    if (rows > 1 && !n_new) return fail("m2f_crf_filter: a chunk (rows > 1) needs n_new");
    CrfFilterArgs a;
    a.logits = logits; a.S = S; a.C = C; a.rows = rows; a.params = params; a.count = count; a.active = active; a.n_new = n_new; a.phi = phi;
    M2F_HIP(m2f_launch_crf_filter(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_supcon_scratch_floats(int N, int D) { return (int64_t)m2f_supcon_ws_floats(N, D); }

int m2f_supcon(int N, int D, int C, const float* features, int ld, const int64_t* labels, const float* class_w, const float* hyper_dev,
               float* scratch, float* row_terms, float* dfeatures, int ldd, m2f_stream_t stream) {
    if (!features || !labels || !hyper_dev || !scratch || !row_terms || !dfeatures)
        return fail("m2f_supcon: NULL features / labels / hyper_dev / scratch / row_terms / dfeatures");
    if (N < 1 || D < 1 || C < 1 || ld < D || ldd < D) return fail("m2f_supcon: N >= 1, D >= 1, C >= 1, ld >= D and ldd >= D required");
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) || (reinterpret_cast<uintptr_t>(row_terms) & 15)) return fail("m2f_supcon: scratch and row_terms must be 16-byte aligned");
    SupconArgs a;
    a.feat = features; a.N = N; a.D = D; a.ld = ld; a.labels = labels; a.C = C; a.class_w = class_w; a.hyper = hyper_dev;
    a.ws = scratch; a.row_terms = row_terms; a.dfeat = dfeatures; a.ldd = ldd;
    M2F_HIP(m2f_launch_supcon(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_adv_scratch_bytes(int T) {
    if (T < 1) { fail("m2f_adv_scratch_bytes: T >= 1 required"); return -1; }
    return (int64_t)m2f_adv_slices(T) * 3 * (int64_t)sizeof(double);
}

// what both stand-alone entries of the adversarial ascent ask of their rows; nullptr: fine
static const char* adv_shape_error(int T, int d, int ld) {
    if (T < 1 || d < 1) return "T >= 1 and d >= 1 required";
    if ((ld & 3) || ld < ((d + 3) & ~3)) return "rows must be 16-byte aligned: ld a multiple of 4, >= d rounded up to 4";
    if ((int64_t)T * d >= ((int64_t)1 << 32)) return "T * d must stay below 2^32";
    return nullptr;
}

int m2f_adv_ascend(int T, int d, int ld, const float* x_clean, const float* g, float* delta, float* x, const uint8_t* key_pad,
                   const float* hyper_dev, int norm_kind, void* scratch, m2f_stream_t stream) {
    if (const char* e = adv_shape_error(T, d, ld)) return fail(std::string("m2f_adv_ascend: ") + e);
    if (!x_clean || !delta || !x || !key_pad || !hyper_dev) return fail("m2f_adv_ascend: NULL x_clean / delta / x / key_pad / hyper_dev");
    if (norm_kind != 0 && norm_kind != 1) return fail("m2f_adv_ascend: norm_kind is 0 (utterance) or 1 (batch)");
    if (norm_kind == 1 && (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 15))) return fail("m2f_adv_ascend: the batch norm needs 16-byte aligned scratch of m2f_adv_scratch_bytes bytes");
    if ((reinterpret_cast<uintptr_t>(x_clean) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(delta) | reinterpret_cast<uintptr_t>(x)) & 15)
        return fail("m2f_adv_ascend: x_clean, g, delta and x must be 16-byte aligned");
    if (x == x_clean || delta == x || delta == x_clean || (g && (g == delta || g == x))) return fail("m2f_adv_ascend: x_clean, g, delta and x must be four buffers");
    AdvArgs a{};
    a.T = T; a.d = d; a.ld = ld; a.x_clean = x_clean; a.g = g; a.delta = delta; a.x = x; a.skip = key_pad; a.hyper = hyper_dev;
    a.partial = static_cast<double*>(scratch);
    M2F_HIP(m2f_launch_adv_ascend(a, norm_kind, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_adv_init(int T, int d, int ld, float* delta, const uint8_t* key_pad, float init_mag, const uint32_t* rng_state, uint32_t site,
                 m2f_stream_t stream) {
    if (const char* e = adv_shape_error(T, d, ld)) return fail(std::string("m2f_adv_init: ") + e);
    if (!delta || !key_pad || !rng_state) return fail("m2f_adv_init: NULL delta / key_pad / rng_state");
    if (!(init_mag >= 0.f) || !std::isfinite(init_mag)) return fail("m2f_adv_init: init_mag must be a finite number >= 0");
    const float scale = (float)((double)init_mag / std::sqrt((double)d));
    M2F_HIP(m2f_launch_adv_init(delta, T, d, ld, key_pad, scale, rng_state, site, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_aux_head_scratch_floats(int N, int D, int A) { return (int64_t)m2f_aux_head_ws_floats(N, D, A); }

// what every stand-alone entry of the auxiliary head asks of its shapes and feature rows; nullptr: fine
static const char* aux_head_shape_error(int N, int D, int A, const float* features, int ld, const float* params, const float* scratch) {
    if (N < 1 || D < 1 || D > 1024) return "N >= 1 and 1 <= D <= 1024 required";
    if (A < 2 || A > 16) return "2 <= A <= 16 auxiliary classes required";
    if (!features || !params || !scratch) return "NULL features / params / scratch";
    if (ld < ((D + 3) & ~3) || (ld & 3) || (reinterpret_cast<uintptr_t>(features) & 15)) return "feature rows must be 16-byte aligned: ld a multiple of 4, >= D rounded up to 4";
    if ((reinterpret_cast<uintptr_t>(params) & 15) || (reinterpret_cast<uintptr_t>(scratch) & 15)) return "params and scratch must be 16-byte aligned";
    return nullptr;
}

int m2f_aux_head(int N, int D, int A, int C, const float* features, int ld, const float* params, const int64_t* labels,
                 const int64_t* aux_labels, const float* class_w, const float* hyper_dev, float* scratch, float* aux_logits,
                 float* row_terms, float* dfeatures, int ldd, float* dparams, m2f_stream_t stream) {
    if (const char* e = aux_head_shape_error(N, D, A, features, ld, params, scratch)) return fail(std::string("m2f_aux_head: ") + e);
    if (!labels || !aux_labels || !hyper_dev || !aux_logits || !row_terms || !dfeatures) return fail("m2f_aux_head: NULL labels / aux_labels / hyper_dev / aux_logits / row_terms / dfeatures");
    if (C < 1 || ldd < ((D + 3) & ~3) || (ldd & 3) || (reinterpret_cast<uintptr_t>(dfeatures) & 15)) return fail("m2f_aux_head: C >= 1 and 16-byte aligned dfeatures rows (ldd a multiple of 4, >= D rounded up to 4) required");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* g = scratch;
    float* part = g + (size_t)N * 16 + (((size_t)N + 3) & ~(size_t)3);
    AuxHeadArgs a;
    a.feat = features; a.N = N; a.D = D; a.ld = ld; a.params = params; a.A = A; a.labels = labels; a.C = C; a.class_w = class_w;
    a.aux_labels = aux_labels; a.hyper = hyper_dev; a.aux_logits = aux_logits; a.ldu = A; a.g = g; a.row_term = row_terms;
    M2F_HIP(m2f_launch_aux_rows(a, s));
    M2F_HIP(m2f_launch_aux_join(dfeatures, ldd, nullptr, 0, g, 16, params, A, N, D, nullptr, hyper_dev, 1.f, 0, 0, ShadowMap{nullptr, nullptr, 0}, s));
    if (dparams) M2F_HIP(m2f_launch_aux_param_grad(features, ld, g, 16, A, N, D, part, nullptr, hyper_dev, dparams, s));
    return 0;
}

int m2f_aux_head_forward(int N, int D, int A, const float* features, int ld, const float* params, float* scratch, float* logits,
                         m2f_stream_t stream) {
    // (scratch is not used by the forward: accepted for symmetry with the other entries, may be NULL)
    if (const char* e = aux_head_shape_error(N, D, A, features, ld, params, features)) return fail(std::string("m2f_aux_head_forward: ") + e);
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail("m2f_aux_head_forward: scratch must be 16-byte aligned or NULL");
    if (!logits) return fail("m2f_aux_head_forward: NULL logits");
    AuxHeadArgs a{};
    a.feat = features; a.N = N; a.D = D; a.ld = ld; a.params = params; a.A = A; a.aux_logits = logits; a.ldu = A;
    M2F_HIP(m2f_launch_aux_rows(a, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_aux_head_backward(int N, int D, int A, const float* features, int ld, const float* params, const float* g, float* scratch,
                          float* dfeatures, int ldd, float* dparams, m2f_stream_t stream) {
    if (const char* e = aux_head_shape_error(N, D, A, features, ld, params, scratch)) return fail(std::string("m2f_aux_head_backward: ") + e);
    if (!g) return fail("m2f_aux_head_backward: NULL g");
    if (dfeatures && (ldd < ((D + 3) & ~3) || (ldd & 3) || (reinterpret_cast<uintptr_t>(dfeatures) & 15))) return fail("m2f_aux_head_backward: dfeatures rows must be 16-byte aligned (ldd a multiple of 4, >= D rounded up to 4)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = scratch + (size_t)N * 16 + (((size_t)N + 3) & ~(size_t)3);
    if (dfeatures) M2F_HIP(m2f_launch_aux_join(dfeatures, ldd, nullptr, 0, g, A, params, A, N, D, nullptr, nullptr, 1.f, 0, 0, ShadowMap{nullptr, nullptr, 0}, s));
    if (dparams) M2F_HIP(m2f_launch_aux_param_grad(features, ld, g, A, A, N, D, part, nullptr, nullptr, dparams, s));
    return 0;
}

int m2f_aux_head_join(int N, int D, int A, float* dh, int ldd, const float* h, int ld, const float* g, int ldg, const float* params,
                      const float* scale_dev, const float* hyper_dev, float gate_scale, int add, uint16_t* shadow, m2f_stream_t stream) {
    if (N < 1 || D < 1 || D > 1024) return fail("m2f_aux_head_join: N >= 1 and 1 <= D <= 1024 required");
    if (A < 2 || A > 16) return fail("m2f_aux_head_join: 2 <= A <= 16 auxiliary classes required");
    if (!dh || !g || !params || ldg < A) return fail("m2f_aux_head_join: NULL dh / g / params, or ldg < A");
    auto rows_bad = [&](const float* p, int l) { return l < ((D + 3) & ~3) || (l & 3) || (reinterpret_cast<uintptr_t>(p) & 15); };
    if (rows_bad(dh, ldd) || (h && rows_bad(h, ld))) return fail("m2f_aux_head_join: dh and h rows must be 16-byte aligned (row strides multiples of 4, >= D rounded up to 4)");
    if (reinterpret_cast<uintptr_t>(params) & 15) return fail("m2f_aux_head_join: params must be 16-byte aligned");
    // (the caller's shadow maps dh element for element, as the plan's activation shadow maps its workspace)
    const ShadowMap sh{shadow ? dh : nullptr, shadow, shadow ? (size_t)N * ldd : 0};
    M2F_HIP(m2f_launch_aux_join(dh, ldd, h, ld, g, ldg, params, A, N, D, scale_dev, hyper_dev, gate_scale, add, shadow ? 1 : 0, sh, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_w2v_conv0_scratch_floats(int B, int C, int T0) {
    return B < 1 || C < 1 || T0 < 1 ? 0 : (int64_t)2 * B * C * (m2f_w2v_conv0_chunks(T0) + 1);
}

int m2f_w2v_conv0(int B, int N, const float* wave, const float* w0, int k0, int s0, int C, int T0, int P0, const float* gamma,
                  const float* beta, float eps, float* scratch, float* out32, uint16_t* out16, m2f_stream_t stream) {
    if (!wave || !w0 || !gamma || !beta || !scratch || !out32 == !out16) return fail("m2f_w2v_conv0: NULL operand, or not exactly one output");
    if (k0 < 1 || k0 > M2F_W2V_CONV0_MAX_TAPS || s0 < 1 || s0 > M2F_W2V_CONV0_MAX_STRIDE) return fail("m2f_w2v_conv0: kernel <= 16 and stride <= 8 only");
    if (B < 1 || C < 1 || N < k0 || T0 != (N - k0) / s0 + 1 || P0 < T0) return fail("m2f_w2v_conv0: T0 must be (N - k0) / s0 + 1 and P0 >= T0");
    float* stats = scratch + (int64_t)2 * B * C * m2f_w2v_conv0_chunks(T0);
    M2F_HIP(m2f_launch_w2v_conv0(wave, B, N, w0, k0, s0, C, T0, P0, gamma, beta, eps, scratch, stats, out32, out16,
                                 static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_w2v_feat_layernorm(int B, int S, int P, int C, const float* x, const float* gamma, const float* beta, float eps, float* out32,
                           uint16_t* out16, m2f_stream_t stream) {
    if (!x || !gamma || !beta || !out32) return fail("m2f_w2v_feat_layernorm: NULL operand");
    if (B < 1 || S < 1 || P < S || C < 1 || C > M2F_W2V_FEAT_MAX_C) return fail("m2f_w2v_feat_layernorm: need S <= P and 1 <= C <= 1024");
    M2F_HIP(m2f_launch_w2v_feat_ln(x, B, S, P, C, gamma, beta, eps, out32, out16, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_w2v_pos_conv(int B, int S, int d, int groups, int K, const float* x, const int32_t* lengths, const void* w, const float* bias,
                     float* out, int bf16, m2f_stream_t stream) {
    if (!x || !lengths || !w || !bias || !out) return fail("m2f_w2v_pos_conv: NULL operand");
    if (B < 1 || S < 1 || groups < 1 || d % groups || (d / groups) % 16 || d / groups > 64 || K < 1 || K > M2F_W2V_POS_MAX_TAPS)
        return fail("m2f_w2v_pos_conv: channels per group must be 16, 32, 48 or 64 and 1 <= K <= 256");
    if (x == out) return fail("m2f_w2v_pos_conv: out must not alias x");
    M2F_HIP(m2f_launch_w2v_pos_conv(x, lengths, B, S, d, groups, K, w, bias, out, bf16 != 0, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_w2v_masked_mean(int B, int S, int d, const float* x, const int32_t* lengths, float* out, m2f_stream_t stream) {
    if (!x || !lengths || !out || B < 1 || S < 1 || d < 1) return fail("m2f_w2v_masked_mean: NULL operand or empty shape");
    M2F_HIP(m2f_launch_w2v_masked_mean(x, lengths, B, S, d, out, static_cast<hipStream_t>(stream)));
    return 0;
}

int64_t m2f_mel_frontend_scratch_floats(int B) {
    return B < 1 ? 0 : (int64_t)(B + 63) / 64 * 64 + (int64_t)B * M2F_MEL_FRAMES * M2F_MEL_BANDS;
}

int m2f_mel_frontend(int B, int N, const float* wave, const int32_t* lengths, const float* basis, const float* fbT, int png_levels,
                     float* scratch, float* img, m2f_stream_t stream) {
    if (!wave || !lengths || !basis || !fbT || !scratch || !img) return fail("m2f_mel_frontend: NULL operand");
    if (B < 1 || N < 1) return fail("m2f_mel_frontend: empty batch");
    float* logmel = scratch + (int64_t)(B + 63) / 64 * 64;
    M2F_HIP(m2f_launch_mel_frontend(wave, lengths, B, N, basis, fbT, png_levels != 0, scratch, logmel, img, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_mel_stem(int B, const float* img, const float* w, const float* bias, float* out32, uint16_t* out16, m2f_stream_t stream) {
    if (!img || !w || !bias || !out32 == !out16) return fail("m2f_mel_stem: NULL operand, or not exactly one output");
    if (B < 1) return fail("m2f_mel_stem: empty batch");
    M2F_HIP(m2f_launch_mel_stem(img, B, w, bias, out32, out16, static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_mel_conv(int B, int H, int W, int Cin, int Cout, int ks, int stride, const void* x, const void* w, const float* bias,
                 const void* res, void* out, int bf16, int out_fp32, int relu, m2f_stream_t stream) {
    if (!x || !w || !bias || !out) return fail("m2f_mel_conv: NULL operand");
    if (B < 1 || H < 1 || W < 1 || Cin < 32 || Cin % 32 || Cout < 64 || Cout % 64 || (ks != 1 && ks != 3) || stride < 1 || stride > 2)
        return fail("m2f_mel_conv: Cin a multiple of 32, Cout a multiple of 64, 1x1 or 3x3 windows, stride 1 or 2");
    if (out == x || (res && out == res)) return fail("m2f_mel_conv: out must not alias x or res");
    const int pad = ks / 2, Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    if ((int64_t)B * Ho * Wo > (1 << 30)) return fail("m2f_mel_conv: more than 2^30 output pixels in one launch");
    M2F_HIP(m2f_launch_mel_conv(x, w, bias, res, out, B, H, W, Cin, Cout, ks, stride, bf16 != 0, out_fp32 != 0, relu != 0,
                                static_cast<hipStream_t>(stream)));
    return 0;
}

int m2f_mel_head(int B, int HW, int C, const void* x, int bf16_in, const float* w1t, const float* b1, int N1, const float* w2t,
                 const float* b2, int N2, float* out, m2f_stream_t stream) {
    if (!x || !w1t || !b1 || !w2t || !b2 || !out) return fail("m2f_mel_head: NULL operand");
    if (B < 1 || HW < 1 || C < 1 || N1 < 1 || N2 < 1 || N2 > 512 || (C + N1) * 4 > 64 * 1024)
        return fail("m2f_mel_head: need N2 <= 512 and C + N1 floats of LDS at most 64 KiB");
    M2F_HIP(m2f_launch_mel_head(x, bf16_in != 0, B, HW, C, w1t, b1, N1, w2t, b2, N2, out, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"
