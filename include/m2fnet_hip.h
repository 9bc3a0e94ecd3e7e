/* m2fnet_hip.h - C ABI of the MI355X-native M2FNet fusion-transformer training path.
 *
 * Shared library: multimodal-emotion-recognition_amd/csrc/libm2fnet_hip.so (gfx950 only).
 * Plain pointers, sizes and a hipStream_t only - no torch types.  All device buffers are owned by the
 * caller (the Python host allocates them as torch tensors; any hipMalloc'ed memory works).  Every
 * function returns 0 on success and a non-zero code on failure (m2f_last_error() has the text); the
 * Python binding turns non-zero into an exception.  One stream per rank, no internal threads, no
 * allocation inside the library.
 *
 * The reference (iosonopersia/Multimodal-Emotion-Recognition) has no FFI: its "interface" for this path
 * is the Python surface of src/model.py / src/train.py.  Each entry point below names the reference
 * code it stands in for (paths relative to the reference root).
 */
#ifndef M2FNET_HIP_H
#define M2FNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* m2f_stream_t;            /* hipStream_t */
typedef struct m2f_plan m2f_plan;

/* Plain-value mirror of the reference's `config.model` sub-tree (src/config.yaml:31-54, consumed at
 * src/model.py:28-56).  dim_ff / ln_eps are the torch defaults the reference inherits (2048, 1e-5). */
typedef struct m2f_config {
    int32_t audio_enabled, text_enabled, fam_enabled;
    int32_t d_audio, d_text, d_fam;
    int32_t nhead_audio, nhead_text, nhead_fam;
    int32_t nlayers_audio, nlayers_text, nlayers_fam;   /* n_encoder_layers, n_encoder_layers, FAM.n_layers */
    int32_t ntrans_audio, ntrans_text;                  /* n_transformers */
    int32_t cls_hidden, cls_out, cls_layers;
    int32_t dim_ff;
    float dropout;
    float ln_eps;
} m2f_config;

enum { M2F_F32 = 0, M2F_BF16 = 1 };    /* GEMM operand precision: exact-fp32 MFMA | bf16 MFMA (fp32 accumulate) */

/* Buffers inside the caller-provided workspace that the host reads / writes (m2f_plan_buffer). */
enum {
    M2F_BUF_TEXT = 0,       /* float [B*L, pad8(d_text)]  input (batch["text"], src/train.py:222); rows padded to x8  */
    M2F_BUF_AUDIO = 1,      /* float [B*L, pad8(d_audio)] input (batch["audio"], src/train.py:223); pad columns stay 0 */
    M2F_BUF_KEYPAD = 2,     /* uint8 [B*L]           input  (batch["padding_mask"], 1 = pad, :225)      */
    M2F_BUF_LABELS = 3,     /* int64 [B*L]           input  (batch["emotion"], -1 = ignore, :224)       */
    M2F_BUF_CLASSW = 4,     /* float [16]            input  optional class weights (src/train.py:45-48) */
    M2F_BUF_LOGITS = 5,     /* float [B*L, cls_out]  output (M2FNet.forward, src/model.py:145)          */
    M2F_BUF_LOSS = 6,       /* float [4]: loss, denominator, numerator, - ; for train plans this IS grads[total..] */
    M2F_BUF_DLOGITS = 7,    /* float [B*L, cls_out]  d loss / d logits (written by m2f_loss, or by host) */
    M2F_BUF_FAM0_OUT = 8,   /* float [B*L, pad8(d_fam)] first fusion layer output (kernel-level parity)  */
    M2F_BUF_CU_SEQLENS = 9, /* int32 [B+1]           input of PACKED plans: dialogue b owns token rows cu[b] .. cu[b+1]-1 */
    M2F_BUF_DTEXT = 10,     /* float [B*L, pad8(d_text)]  output d loss / d text (text.grad, src/model.py:115-119; train plans, m2f_plan_backward_outputs) */
    M2F_BUF_DAUDIO = 11,    /* float [B*L, pad8(d_audio)] output d loss / d audio (audio.grad, src/model.py:103-107; same rows as M2F_BUF_AUDIO)  */
    M2F_BUF_STREAM_LEN = 12,    /* int32 [S]  stream plans: utterances cached per stream slot (advanced by m2f_stream_step, zeroed by m2f_stream_reset) */
    M2F_BUF_STREAM_ACTIVE = 13, /* uint8 [S]  stream plans, input: 1 = the slot takes an utterance in the next m2f_stream_step */
    M2F_BUF_STREAM_NEW = 14,    /* int32 [S]  chunk plans, input: utterances (0 .. T) the slot takes in the next m2f_stream_prefill */
    M2F_BUF_STREAM_TABLE = 15,  /* int32 [S, ceil(C / page_rows)]  paged stream plans, input: the page of each run of page_rows cache rows of a slot (a chunk plan: its parent's) */
    M2F_BUF_TEACHER = 16,       /* float [B*L, cls_out]  train plans, input of the distillation criterion: the teacher's logits, token rows as M2F_BUF_LOGITS */
    M2F_BUF_DISTILL = 17,       /* float [2]  train plans, input of the distillation criterion: alpha, tau (read on the device at every step) */
    M2F_BUF_STREAM_ATTN = 18,   /* float [sites][S][H_site][C]  stream plans with m2f_plan_stream_attention on: the caller's buffer (NULL: off) */
    M2F_BUF_SPEAKERS = 19,      /* uint8 [T]  input of a plan with speaker heads (m2f_plan_attention_speakers): the speaker id of every token row, in the plan's token order (padded: [B*L] as M2F_BUF_KEYPAD; packed: row cu[b] + i); stream plans: [S], chunk plans [S*T] - the new utterances' ids */
    M2F_BUF_STREAM_SPEAKERS = 20,   /* uint8 [S][C]  stream plans with speaker heads: the caller's buffer of cached speaker ids by logical cache row (m2f_plan_stream_speakers; NULL: none) */
    M2F_BUF_FOCAL = 21,         /* float [1]  train and eval plans, input of the focal criterion (m2f_plan_focal): gamma (read on the device at every step) */
    M2F_BUF_PARTNER = 22,       /* int32 [T]  train plans, input of the R-Drop criterion (m2f_plan_rdrop): the twin of every token row, in the plan's token order (as M2F_BUF_CU_SEQLENS is an input), or -1 */
    M2F_BUF_RDROP = 23,         /* float [1]  train plans, input of the R-Drop criterion: alpha (read on the device at every step) */
    M2F_BUF_SUPCON = 24,        /* float [2]  train plans, input of the supervised contrastive criterion (m2f_plan_supcon): (lambda, tau), read on the device at every step */
    M2F_BUF_FEATURES = 25,      /* float [T, pad8(cls_hidden)]  the classifier's last hidden activation as stored (post-ReLU, post-dropout in train mode; the A operand of the final Linear), in the plan's token order - what m2f_plan_supcon contrasts; read-only for the caller */
    M2F_BUF_COUNT = 26,         /* the ids above; kept at its value for callers built against it - M2F_BUF_END bounds m2f_plan_buffer's ids */
    M2F_BUF_AUX = 26,           /* float [2]  train plans, input of the auxiliary label head (m2f_plan_aux_head): (lambda, eps_a), read on the device at every step */
    M2F_BUF_AUX_LABELS = 27,    /* int64 [T]  train plans, input of the auxiliary label head: the second label of every token row, in the plan's token order (as M2F_BUF_LABELS); a value outside [0, num_aux) = ignored */
    M2F_BUF_AUX_LOGITS = 28,    /* float [T, 16]  train plans, the auxiliary head's logits of the last step (columns 0 .. num_aux-1 of every row); read-only for the caller */
    M2F_BUF_END = 29,           /* the ids above; kept at its value for callers built against it - M2F_BUF_LIMIT bounds m2f_plan_buffer's ids */
    /* the adversarial state of a plan (m2f_plan_adversarial): pointers into the CALLER's state buffer, NULL while it is off */
    M2F_BUF_ADV = 29,           /* float [2]  (epsilon, step_size) of the ascent, read on the device by every m2f_plan_adv_ascend / m2f_plan_adv_begin */
    M2F_BUF_ADV_SKIP = 30,      /* uint8 [T]  input: 1 = the token row is padding or a filler row - the ascent neither reads it for a norm nor writes it */
    M2F_BUF_ADV_DELTA_TEXT = 31,    /* float [T, pad8(d_text)]   the perturbation of the text rows (token rows as M2F_BUF_TEXT); NULL: not asked for */
    M2F_BUF_ADV_DELTA_AUDIO = 32,   /* float [T, pad8(d_audio)]  the perturbation of the audio rows */
    M2F_BUF_LIMIT = 33
};
/* the hash sites of the uniform start of the perturbation (m2f_adv_init): far above every dropout site a plan hands out (1, 2, ...) */
#define M2F_ADV_SITE_TEXT 0xAD510001u
#define M2F_ADV_SITE_AUDIO 0xAD510002u

const char* m2f_last_error(void);
int m2f_device_check(void);            /* 0 iff the current HIP device is gfx950 */

/* Flat parameter layout = reference state_dict order (src/model.py:24-100), unique tensors
 * only, each padded to 64 floats.  Fills offsets/numels (elements) for up to max_entries tensors and
 * *total (flat length in elements); returns the number of unique tensors, or <0 on error. */
int m2f_param_layout(const m2f_config* cfg, int64_t* offsets, int64_t* numels, int max_entries, int64_t* total);

/* Workspace size (bytes) a plan for (cfg, B dialogues, L utterances) needs. */
int64_t m2f_workspace_bytes(const m2f_config* cfg, int B, int L, int train);

/* A plan = the launch list of one M2FNet step for fixed (cfg, B, L, precision, train/eval) bound to the
 * caller's flat parameter buffer, flat gradient buffer (may be NULL for eval plans), workspace and
 * dropout RNG state (4 x uint32 in device memory: seed_lo, seed_hi, step_lo, step_hi).
 * The gradient buffer must hold total + 64 floats (total from m2f_param_layout): the 64-float tail receives
 * (loss, denominator, numerator) so that a data-parallel all-reduce of the whole buffer also sums the
 * valid-utterance denominators. */
m2f_plan* m2f_plan_create(const m2f_config* cfg, int B, int L, int precision, int train,
                          float* params, float* grads, void* workspace, int64_t workspace_bytes,
                          uint32_t* rng_state);
/* PACKED ("varlen") plan: the T token rows of every buffer belong to B dialogues of 1 .. L utterances each, dialogue b owning rows
 * cu[b] .. cu[b+1]-1 of M2F_BUF_CU_SEQLENS (int32 [B+1], cu[0] = 0, cu[B] <= T, written by the caller before each step; rows from
 * cu[B] on are padding: label -1, finite inputs).  No pad slots inside dialogues, so a ragged batch (reference collate_fn,
 * src/dataset.py:69-89, pads every dialogue to the longest) costs its valid utterances only.  M2F_BUF_KEYPAD is not read.
 * Same arithmetic per valid utterance as the padded plan of the same dialogues; B <= T <= B * L.
 * L (the longest dialogue the plan holds) may be 1 .. 512 here, against 1 .. 64 for the padded plans: above 64 the dialogue
 * attention runs on the long-dialogue kernels (m2f_attention_varlen_*), and B * H * L * L must stay below 2^32 for every
 * attention site's head count H (the dropout keep index is 32-bit). */
int64_t m2f_workspace_bytes_packed(const m2f_config* cfg, int B, int L, int T, int train);
m2f_plan* m2f_plan_create_packed(const m2f_config* cfg, int B, int L, int T, int precision, int train,
                                 float* params, float* grads, void* workspace, int64_t workspace_bytes,
                                 uint32_t* rng_state);
/* SHARED PARAMETER SHADOWS (bf16 mode).  The GEMMs stage bf16 copies of every 2-D parameter (W [rows][pad8(cols)] and W^T
 * [cols][pad8(rows)]); a plan of m2f_plan_create keeps its own copies in its workspace and refreshes them with cast launches at
 * the head of every forward.  With m2f_plan_create_shared all plans of a model use ONE caller-owned buffer of
 * m2f_param_shadow_elems(cfg) uint16 (256-byte aligned; initialise it once with m2f_param_shadow_init), and an optimizer step
 * through m2f_adam_step_shadowed writes the shadows of the parameters it has just updated.  The caller then declares them
 * current with m2f_plan_params_fresh(plan, 1) and the forward skips its parameter casts (2 x 87 us of 2.7 ms at C3); after
 * any OTHER write to the parameters (load_state_dict, a foreign optimizer) it must pass 0 again - a forward that ran the casts
 * leaves the shadows current, too.  T = 0: padded plan (L <= 64), T > 0: packed plan of T token rows (as m2f_plan_create_packed,
 * L <= 512).
 * No counterpart in the reference: torch keeps no low-precision parameter copies (src/train.py:56,231 is all it does). */
int64_t m2f_param_shadow_elems(const m2f_config* cfg);
int m2f_param_shadow_init(const m2f_config* cfg, uint16_t* param_shadow, m2f_stream_t stream);
int64_t m2f_workspace_bytes_shared(const m2f_config* cfg, int B, int L, int T, int train);
m2f_plan* m2f_plan_create_shared(const m2f_config* cfg, int B, int L, int T, int precision, int train,
                                 float* params, float* grads, void* workspace, int64_t workspace_bytes,
                                 uint32_t* rng_state, uint16_t* param_shadow);
int m2f_plan_params_fresh(m2f_plan* plan, int fresh);
void m2f_plan_destroy(m2f_plan* plan);
void* m2f_plan_buffer(m2f_plan* plan, int which);
int m2f_plan_num_launches(m2f_plan* plan, int phase);   /* 0 fwd, 1 loss, 2 bwd */

/* M2FNet.forward (src/model.py:102-145): inputs read from M2F_BUF_TEXT/AUDIO/KEYPAD, logits -> M2F_BUF_LOGITS. */
int m2f_forward(m2f_plan* plan, m2f_stream_t stream);
/* criterion(outputs.permute(0,2,1), emotion) (src/train.py:229; CrossEntropyLoss(ignore_index=-1,
 * label_smoothing) of :48-50): labels from M2F_BUF_LABELS, loss -> M2F_BUF_LOSS, dlogits -> M2F_BUF_DLOGITS.
 * normalise=1: gradient of the mean-over-valid loss; 0: gradient of the SUM (data-parallel path divides
 * by the global denominator after the all-reduce). */
int m2f_loss(m2f_plan* plan, float label_smoothing, int use_class_weights, int normalise, m2f_stream_t stream);
/* loss.backward() (src/train.py:230): consumes M2F_BUF_DLOGITS, OVERWRITES the flat gradient buffer. */
int m2f_backward(m2f_plan* plan, m2f_stream_t stream);
/* What m2f_backward computes (loss.backward() reaching `text` / `audio` as autograd leaves, src/model.py:106-119, and / or the
 * parameters).  input_mask: 1 = d loss / d text into M2F_BUF_DTEXT, 2 = d loss / d audio into M2F_BUF_DAUDIO (token rows as the
 * input staging buffers; an enabled modality only): the backward chain runs on through the QKV in-projection of the first encoder
 * layer of stack 0 (the outer skip x + enc(x) included) - one more dgrad launch behind the branch chains, both modalities grouped.
 * param_grads = 0: no weight gradients, no LayerNorm-parameter reduces, the flat gradient buffer is never written (a train plan
 * created with grads = NULL starts so and cannot switch to 1); m2f_step, m2f_step_part, m2f_plan_fused_adam_setup and
 * m2f_plan_grad_bf16 then fail.  Default (0, 1): the backward of m2f_plan_create as before, launch for launch; the parameter
 * gradients are bit-identical with input gradients on.  A change rebuilds every launch list in the same workspace and destroys the
 * captured graphs (fused-optimizer and bf16-gradient setups must be repeated); call it between steps, never between a forward and
 * its backward. */
int m2f_plan_backward_outputs(m2f_plan* plan, int input_mask, int param_grads);
/* Context band of EVERY attention site of the plan - both modality encoders and every fusion layer, forward and backward (one
 * unmasked site would leak the future): utterance i attends to utterances i - past .. i + future of its dialogue, each side >= 0
 * or negative = unlimited (m2f_attn_opts below has the rule and the rows that see no key).  (-1, 0): causal, the online
 * setting of emotion recognition in conversation; (-1, -1), the default: the reference's offline attention, bit for bit what the plan
 * computed before this entry existed.  No counterpart in the reference (its modules take no attn_mask).  Pad slots under a band
 * are not the reference's numbers (as the pad slots of packed plans).  A change destroys the captured graphs; call it between
 * steps, never between a forward and its backward.  m2f_plan_get_attention_band reads the setting back (-1 = unlimited). */
int m2f_plan_attention_band(m2f_plan* plan, int past, int future);
int m2f_plan_get_attention_band(m2f_plan* plan, int* past, int* future);
/* Distance-decay bias (ALiBi) of EVERY attention site of the plan: a visible key's score becomes
 * fma(-slope(h, H, gain), float(|i - j|), dot(q_i, k_j) / sqrt(hd)) in fp32, i and j the positions the band compares and slope the
 * fixed geometric recipe of m2f_attn_opts::bias_gain below.  gain >= 0 and finite; 1.0 is ALiBi, 0 (the default) is off and runs the
 * kernels the plan ran before this entry existed.  The APPLIED gain is the requested one rounded to bf16 (the launch descriptor holds
 * 16 bits of it); m2f_plan_get_attention_bias reports the applied value.  No parameters, no change to the saved probabilities' layout:
 * the backward kernels read the probabilities and ignore the setting.  Works on train, eval, packed, stream and chunk plans; on a
 * stream plan before the first step or between steps (the K / V caches do not depend on it).  A chunk plan takes its parent's gain
 * when it is created.  A change destroys the captured graphs; call it between steps, never between a forward and its backward. */
int m2f_plan_attention_bias(m2f_plan* plan, float gain);
int m2f_plan_get_attention_bias(m2f_plan* plan, float* gain);
/* SPEAKER HEADS of EVERY attention site of the plan: at a site with H heads, heads 0 .. n_same - 1 let query utterance i see key j only
 * if speakers[j] == speakers[i] (the utterance itself always qualifies), heads n_same .. n_same + n_other - 1 only if they differ, the
 * other heads are untouched.  The condition is ANDed with key padding and the context band, the distance bias applies to what stays
 * visible; a hidden key has P = 0 exactly, a query that sees no key (an other-speaker head in a monologue) a zero row of P and a zero
 * output row.  At a fusion site (query = text, key = audio) utterance i has one speaker in both roles.  speakers = M2F_BUF_SPEAKERS,
 * uint8, one id per token row in the plan's token order, an INPUT like the mask, written before each forward; only equality is used,
 * ids of pad rows are ignored.  n_same, n_other >= 0 and n_same + n_other <= the heads of every enabled site (refused otherwise, naming
 * the site); (0, 0), the default, is off and runs the kernels the plan ran before this entry existed.  No parameters; the backward
 * kernels read the saved probabilities and ignore the setting.  A change destroys the captured graphs; call it between steps.
 * Stream and chunk plans: m2f_plan_stream_speakers first (the cached ids); a chunk plan takes its parent's setting when it is created. */
int m2f_plan_attention_speakers(m2f_plan* plan, int n_same, int n_other);
int m2f_plan_get_attention_speakers(m2f_plan* plan, int* n_same, int* n_other);
/* Stream plans: the caller-owned array of cached speaker ids, uint8 [S][C], indexed by LOGICAL cache row (row u % C of a ring; the row a
 * page table maps on a paged plan - the array itself is dense), one array for all sites (NULL: none; refused while speaker heads are
 * on).  m2f_stream_step / m2f_stream_prefill of a plan with speaker heads read the new utterances' ids from M2F_BUF_SPEAKERS ([S] /
 * [S*T]) and store them into this array in the launch that advances the counters, BEHIND the last attention launch of the step: on a
 * ring that store overwrites the id of the utterance that has just left the window, which every attention launch of the step - they
 * never read the row the new utterance takes - has seen consistently, as the K / V row.  Destroys the captured graphs. */
int m2f_plan_stream_speakers(m2f_plan* plan, void* buffer);
/* ATTENTION MAPS: what nn.MultiheadAttention(need_weights=True) returns - the reference's fusion module computes them at every layer
 * and throws them away (src/model.py:14) - read out of the pre-dropout probabilities that every attention site of a padded or packed
 * plan saves at every forward (train and eval plans alike; csrc/attention_weights.hip).  m2f_plan_attention_sites: the plan's sites in
 * state_dict order - kind 0 = audio_encoders.{index}.layers.{layer}.self_attn, 1 = text_encoders.{index}.layers.{layer}.self_attn,
 * 2 = fusion_layers.{index}.multihead_attention (layer 0) - with their head count and head dim, up to max_sites of them (any array may
 * be NULL); returns their number.  m2f_plan_attention_weights: the maps of the n_sites listed sites (indices into that list) of the
 * LAST forward / step of the plan into out[i] (host array of device pointers, fp32): [B, H, L, L] (per_head) or [B, L, L] - the fp32 sum
 * over h = 0 .. H - 1 in that order times (float)1 / H, torch's average_attn_weights - with the plan's own B and L; element (b, [h,] i, j)
 * = P of query i, key j of dialogue b, exactly 0 where j is a padded key, where i or j lies behind the dialogue's end (packed plans)
 * or where the plan's context band hides the pair.  Pad-query rows of padded plans hold their softmax numbers, as torch's do; a row
 * that sees no key is zeros (torch: NaN).  Train plans with dropout: the PRE-dropout probabilities (torch returns them post-dropout).
 * Eager, one launch per 64 sites, outside every captured graph; nothing is recaptured and no result of the plan changes.  Stream and
 * chunk plans are refused.  No counterpart in the reference beyond the discarded return value. */
int m2f_plan_attention_sites(m2f_plan* plan, int* kind, int* index, int* layer, int* H, int* hd, int max_sites);
int m2f_plan_attention_weights(m2f_plan* plan, const int* sites, int n_sites, int per_head, float* const* out, m2f_stream_t stream);
/* STREAM plan: online inference under a causal context band (past, 0).  S stream slots, each one live dialogue; a step takes ONE new
 * utterance per active slot (row s of M2F_BUF_TEXT / M2F_BUF_AUDIO, both [S, pad8(d)]; M2F_BUF_STREAM_ACTIVE [S]) and leaves its logits
 * in row s of M2F_BUF_LOGITS [S, cls_out].  Under such a band the K and V rows of an utterance at every attention site depend on
 * earlier utterances only, so each site keeps them in a per-slot cache ([S][H][C][pad(hd)], fp32 or - bf16 mode - bf16 rounded once;
 * csrc/attention_stream.hip has the layout) and a step costs one row per dialogue instead of the whole prefix.  Forward only, no
 * dropout; the launch list is the eval plan's for S rows (same GEMM, LayerNorm and classifier launches) with every attention launch
 * replaced by m2f_attention_stream's kernel.  past < 0: no window - a slot holds at most C utterances (1 <= C <= 512), the caller
 * must not step a slot whose count has reached C (the kernel then writes nothing and returns a zero row); past >= 0: the cache is a
 * ring of C rows, C >= past + 1 (raised to it) - the slot sees its last C - 1 utterances, so C = past + 1 is the band (past, 0)
 * and the stream has no length limit.  The caches cost 2 * sum over sites of S * C * pad(d_site) elements.
 * param_shadow: NULL, or the shared parameter-shadow buffer of m2f_plan_create_shared (bf16 mode; m2f_plan_params_fresh applies).
 * m2f_stream_step: forward + count[s] += active[s]; use_graph = 1 replays one captured graph (single stream, no forks) - everything
 * that varies per call lives in device buffers.  m2f_stream_reset: count[s] = 0 for the slots whose byte in `slot_mask` (device uint8
 * [S]) is non-zero, NULL = every slot; stale cache rows are never read, the live rows are counted from 0 again.
 * The caches belong to the parameter values that wrote them: reset every slot after the parameters change.
 * No counterpart in the reference (it has no incremental inference). */
int64_t m2f_stream_workspace_bytes(const m2f_config* cfg, int S, int C, int past, int precision, int shared);
m2f_plan* m2f_plan_create_stream(const m2f_config* cfg, int S, int C, int past, int precision, float* params, void* workspace,
                                 int64_t workspace_bytes, uint16_t* param_shadow);
int m2f_stream_step(m2f_plan* plan, int use_graph, m2f_stream_t stream);
int m2f_stream_reset(m2f_plan* plan, const uint8_t* slot_mask, m2f_stream_t stream);
int64_t m2f_stream_cache_bytes(m2f_plan* plan);          /* bytes of all K / V caches of the plan */
/* CHUNK plan: the other half of the cache interface - UP TO T NEW UTTERANCES PER SLOT in one call (2 <= T <= 64), for loading a history
 * into the caches at the cost of a forward over S * T rows instead of one launch-bound step per utterance.  It is an eval plan of B = S,
 * L = T rows over the caches and counts of `parent`, a stream plan (it allocates no cache; same configuration, precision, capacity
 * and band: m2f_plan_get_attention_band reports the parent's; the parent must outlive it and is not changed in any way).  Slot s takes
 * its first n[s] rows - rows s*T + t, t < n[s], of M2F_BUF_TEXT / M2F_BUF_AUDIO ([S*T, pad8(d)]); n = M2F_BUF_STREAM_NEW, int32 [S],
 * 0 .. T - and leaves their logits in the same rows of M2F_BUF_LOGITS; rows t >= n[s] must hold finite values, their logits mean
 * nothing.  Every attention site runs m2f_attention_stream_chunk's kernel: row t attends to what the slot has cached and to the
 * chunk's rows <= t under the band, exactly as n[s] steps would, and the rows' K / V are stored for the steps and chunks that
 * follow.  past < 0: count[s] + n[s] <= C is the caller's to ensure (the kernel leaves such a slot untouched and returns zero rows).
 * m2f_stream_prefill: forward + count[s] += n[s]; use_graph = 1 replays one captured graph of the chunk plan's own.  Steps of the
 * parent and chunk calls interleave freely on one HIP stream.  M2F_BUF_STREAM_LEN of a chunk plan is the parent's buffer.
 * m2f_stream_step, m2f_stream_reset and m2f_stream_cache_bytes refuse a chunk plan (the last returns -1: it owns no cache). */
int64_t m2f_stream_chunk_workspace_bytes(m2f_plan* parent, int T, int shared);
m2f_plan* m2f_plan_create_stream_chunk(m2f_plan* parent, int T, float* params, void* workspace, int64_t workspace_bytes,
                                       uint16_t* param_shadow);
int m2f_stream_prefill(m2f_plan* plan, int use_graph, m2f_stream_t stream);
/* PAGED stream plan: the same stream with the cache rows allocated in pages.  Every attention site holds K and V POOLS
 * [n_pages][H][page_rows][pad(hd)] (page_rows = 16, 32 or 64; rows padded and aligned as the dense caches') instead of
 * [S][H][C][pad(hd)], and logical cache row r of slot s - utterance r of a plain cache, utterance u with u % C == r of a ring - is row
 * r % page_rows of page table[s][r / page_rows].  table = M2F_BUF_STREAM_TABLE, int32 [S, ceil(C / page_rows)], an INPUT like the mask:
 * the caller owns the allocation (which pages are free, which slot holds which) and writes the table before the call that needs it.
 * Page ids are shared by all sites: page p is index p of every pool.  A step / chunk call reads only the entries of pages that hold
 * a live row of the slot or take a row of this call, entries e < ceil(min(count + new, C) / page_rows); the rest may hold anything.
 * Ids outside 0 .. n_pages - 1 are clamped into the pool.  Memory follows n_pages, not S: S is limited only by the plan's row-wise
 * and GEMM launches.  Arithmetic, order and results are the dense plan's bit for bit.  m2f_plan_create_stream_chunk accepts a paged
 * parent (its sites then run the paged chunk kernel through the parent's table); m2f_stream_step / _prefill / _reset work as on a
 * dense plan and m2f_stream_cache_bytes returns the pools' bytes.  The table starts as zeros. */
int64_t m2f_stream_paged_workspace_bytes(const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows, int shared);
m2f_plan* m2f_plan_create_stream_paged(const m2f_config* cfg, int S, int C, int past, int precision, int n_pages, int page_rows,
                                       float* params, void* workspace, int64_t workspace_bytes, uint16_t* param_shadow);
/* SNAPSHOT / RESTORE of a stream plan's dialogues (dense or paged; csrc/stream_cache.hip).  The caches are a dialogue's whole state and
 * never change once written, so its live rows plus its count are an exact checkpoint.  The packed format: entry e holds the
 * rows = min(lengths[e], C) live physical rows of slot slots[e] as [site in plan order][K, V][H][rows][pad(hd)] at element
 * row_offsets[e] * W, W = m2f_stream_snapshot_row_elems(plan) = sum over sites of 2 * H * pad(hd); it does not depend on dense / paged,
 * page_rows, S or the slot.  m2f_stream_snapshot_sites writes the (H, hd) of up to max_sites sites in plan order and returns their
 * number.  m2f_stream_gather: caches -> packed for n listed slots; m2f_stream_scatter: packed -> caches and count[slot] = lengths[e]
 * (a paged plan: M2F_BUF_STREAM_TABLE must already name the pages of those rows).  slots, lengths: device int32 [n]; row_offsets:
 * device int64 [n]; packed: 16-byte aligned, packed_elems elements of the caches' type.  One eager launch for all sites (per 64
 * sites), outside the captured step graph - which reads the counts and the table from device buffers and is not recaptured.  Both
 * refuse a chunk plan, as m2f_stream_reset does.  A snapshot belongs to the parameter values that wrote it. */
int64_t m2f_stream_snapshot_row_elems(m2f_plan* plan);
int m2f_stream_snapshot_sites(m2f_plan* plan, int* H, int* hd, int max_sites);
int m2f_stream_gather(m2f_plan* plan, int n, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets, void* packed,
                      int64_t packed_elems, m2f_stream_t stream);
int m2f_stream_scatter(m2f_plan* plan, int n, const int32_t* slots, const int32_t* lengths, const int64_t* row_offsets, const void* packed,
                       int64_t packed_elems, m2f_stream_t stream);
/* ATTENTION ROWS OF A STREAM: which cached utterances did the step's prediction use.  m2f_plan_stream_attention(plan, buffer, elems):
 * from the next step on every attention launch of m2f_stream_step runs the weights-emitting form of its kernel (csrc/attention_stream.hip)
 * and leaves each (slot, head)'s row of probabilities in `buffer` - caller-owned like every buffer a plan uses, fp32, 16-byte aligned,
 * elems >= m2f_stream_attention_elems(plan) = sum over sites of S * H * C - laid out [site in m2f_plan_attention_sites order][S][H][C],
 * column t = the t-th oldest live utterance of the slot (the last live column: the one that has just arrived), zeros behind the live
 * count and in the rows of inactive slots.  buffer = NULL: off again, the kernels the step always ran.  A change drops the captured step
 * once (as m2f_plan_distill does on train plans); the step stays one replayed graph, logits and cache rows keep their bits, and
 * M2F_BUF_STREAM_ATTN reports the buffer.  17.8 MB at C3, S = 64, C = 512.  The chunk kernel has no weights form: m2f_stream_prefill
 * leaves the buffer as it was.  m2f_stream_attention: the rows of the LAST step for the listed sites into out[i] (host array of
 * device pointers) as [S, H, C] (per_head) or [S, C] by the head-average rule of m2f_plan_attention_weights; eager, one launch per 64
 * sites, outside the step graph.  Stream plans only (a chunk plan is refused). */
int64_t m2f_stream_attention_elems(m2f_plan* plan);
int m2f_plan_stream_attention(m2f_plan* plan, float* buffer, int64_t buffer_elems);
int m2f_stream_attention(m2f_plan* plan, const int* sites, int n_sites, int per_head, float* const* out, m2f_stream_t stream);
/* Fused train-step body of src/train.py:228-230 (forward + criterion + backward) with the dropout RNG
 * advanced on the device; use_graph=1 captures the launch list into a hipGraph once and replays it. */
int m2f_step(m2f_plan* plan, float label_smoothing, int use_class_weights, int normalise, int use_graph,
             m2f_stream_t stream);

/* The same step in TWO parts, for data-parallel overlap (no counterpart in the reference, which is single-process):
 *   part 0 = dropout-RNG advance + forward + criterion + the backward chain of the classifier and the fusion stack + every weight
 *            gradient whose operands that chain completes;   part 1 = the encoders' backward + the remaining weight gradients.
 * After part 0 the flat gradient buffer is final from element m2f_plan_split_offset(plan) on (fusion stack + classifier = its
 * tail, and the 64-float loss tail behind it), so a rank can put that bucket's all-reduce on the wire and run part 1 under it.
 * m2f_plan_split_offset returns 0 for plans that cannot be split (fp32 mode, eval plans); parts 0 and 1 must alternate.
 * The split step always writes fp32 gradients: it ignores m2f_plan_fused_adam and m2f_plan_grad_bf16. */
int64_t m2f_plan_split_offset(m2f_plan* plan);
int m2f_step_part(m2f_plan* plan, int part, float label_smoothing, int use_class_weights, int normalise, int use_graph,
                  m2f_stream_t stream);

/* Device-side dialogue batcher: Dataset.__getitem__ + collate_fn / apply_padding (src/dataset.py:32-89, src/utils.py:15-31)
 * on device-resident embedding tables.  Token slot t receives row rows[t] of each table; rows[t] < 0 marks a padded slot
 * (features 0, label -1, key_pad 1).  Outputs may be a plan's staging buffers (row strides ld_text / ld_audio). */
int m2f_gather_dialogues(const float* text_table, int d_text, const float* audio_table, int d_audio,
                         const int64_t* label_table, const int32_t* rows, int T, float* text_out, int ld_text,
                         float* audio_out, int ld_audio, uint8_t* key_pad_out, int64_t* labels_out, m2f_stream_t stream);

/* Measurement aid: one EAGER m2f_step with a hipEvent pair recorded on `stream` around every launch.  Fills, per
 * launch, kinds[] (0/1/2 = grouped GEMM forward/dgrad/wgrad form, 3/4 attention fwd/bwd, 5/6 LayerNorm fwd/bwd,
 * 7 dropout-mask, 8 criterion, 9 LayerNorm-parameter reduce, 10 bf16 casts, 11 / 12 unused;
 * chain launches carry + 32 x their part of the model: 0 modality encoders, 1 fusion stack (FusionAttentionModule, src/model.py:13-20), 2 classifier), ms[]
 * (device time) and flops[] (algorithmic FLOPs of the launch, 0 for row-wise kernels).  Synchronises the stream.  Returns the number of launches, or <0. */
int m2f_step_timed(m2f_plan* plan, float label_smoothing, int use_class_weights, int normalise, m2f_stream_t stream,
                   int max_entries, int* kinds, float* ms, double* flops);

/* Calibration of m2f_step_timed's intervals: the mean device time between the two hipEventRecords of a pair with
 * NOTHING between them (*empty_pair_ms) and with a one-thread kernel between them (*trivial_kernel_pair_ms; needs
 * scratch_rng_state = 4 device uint32, may be NULL to skip), over `pairs` pairs on `stream`.  rocprofv3 reports the
 * kernel's own begin..end; an event interval adds this record/dispatch overhead to it.  Synchronises the stream. */
int m2f_event_overhead(uint32_t* scratch_rng_state, int pairs, float* empty_pair_ms, float* trivial_kernel_pair_ms,
                       m2f_stream_t stream);

/* Advances the dropout RNG state by one step on the device (what nn.Dropout's generator advance is to the
 * reference; m2f_step does it itself). */
int m2f_rng_advance(uint32_t* rng_state, m2f_stream_t stream);

/* optimizer.step() of torch.optim.Adam(lr, weight_decay) (src/train.py:56,231): coupled L2, bias-corrected,
 * over flat buffers of n floats (n % 4 == 0).  grad_scale_ptr (device, nullable): g <- g / *grad_scale_ptr. */
int m2f_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  const float* grad_scale_ptr, m2f_stream_t stream);

/* Same update with the gradients given as bf16 (n values, 8-byte aligned): the data-parallel path can exchange
 * gradients in bf16 over xGMI (half the bytes of the fp32 all-reduce) and feed the reduced buffer straight to the
 * optimizer; parameters and both moments stay fp32.  No counterpart in the reference (single process). */
int m2f_adam_step_g16(float* params, const uint16_t* grads_bf16, float* exp_avg, float* exp_avg_sq, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      const float* grad_scale_ptr, m2f_stream_t stream);

/* The same optimizer step over the WHOLE flat buffers of a model (cfg gives the tensor table), walking the 2-D parameters in
 * 64 x 64 tiles so that the kernel also writes their bf16 shadows (W and W^T) into the shared buffer of m2f_param_shadow_init:
 * 28 B of optimizer traffic + 4 B of shadow writes per parameter instead of 28 B + a separate 8 B cast pass per forward. */
int m2f_adam_step_shadowed(const m2f_config* cfg, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           uint16_t* param_shadow, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           const float* grad_scale_ptr, m2f_stream_t stream);
/* ... over the parameter tensors at flat offsets [first, end) only (both the offset of a tensor; end < 0: to the last one), reading the
 * gradients as fp32 or (grads_bf16 != 0) as bf16 with the same indexing.  This is what lets the data-parallel path - which steps
 * bucket by bucket behind each bucket's all-reduce, on the reduced bf16 buffer when the exchange is bf16 - keep the parameter
 * shadows current as well (dp.GradReducer aligns its buckets to tensor boundaries; optim.FusedAdam.step_ranges). */
int m2f_adam_step_shadowed_range(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg,
                                 float* exp_avg_sq, uint16_t* param_shadow, int64_t first, int64_t end, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int step, const float* grad_scale_ptr, m2f_stream_t stream);

/* Gradient clipping by global L2 norm (torch.nn.utils.clip_grad_norm_, norm_type 2) without touching the gradients: the norm of the
 * flat gradient buffer is reduced on the device and the clip is folded into the divisor the optimizer entry points above read as
 * *grad_scale_ptr.  No counterpart in the reference, whose loop does not clip; the rule is torch's.
 *
 * m2f_grad_sumsq: float64 sums of squares of the parameter tensors at flat offsets [first, end) (as m2f_adam_step_shadowed_range:
 * both the offset of a tensor; end < 0: to the last one) of `grads` - fp32, or (grads_bf16 != 0) bf16 with the same indexing;
 * 16-byte aligned - into `scratch` (m2f_grad_norm_scratch_bytes(cfg) bytes, 8-byte aligned): one partial per slice of 8192 elements
 * of one tensor.  Only parameter elements are read: the alignment pads between tensors may hold anything.  Calls over disjoint
 * ranges fill disjoint partials (the data-parallel path may sum bucket by bucket).  grid: workgroups of the launch, <= 0 = default
 * (at most 2048); nontemporal != 0: nontemporal loads.  Neither changes a bit of the result: a partial depends on its slice alone.
 *
 * m2f_grad_norm_finalize: sums EVERY partial of cfg in index order (the caller has covered all tensors) and writes four floats,
 * computed in float64 and rounded once each:
 *   record[0] = norm    = sqrt(sum of squares) / den        den = *den_ptr, or 1 when den_ptr is NULL
 *   record[1] = coef    = min(1, max_norm / (norm + 1e-6))
 *   record[2] = divisor = den if coef == 1 (den's bits), else den / coef         -> pass &record[2] as grad_scale_ptr
 *   record[3] = sqrt(sum of squares)
 * A non-finite norm gives a non-finite coef and divisor (torch's error_if_nonfinite=False).  Same bits on every run. */
int64_t m2f_grad_norm_scratch_bytes(const m2f_config* cfg);
int m2f_grad_sumsq(const m2f_config* cfg, const void* grads, int grads_bf16, int64_t first, int64_t end, double* scratch, int grid,
                   int nontemporal, m2f_stream_t stream);
int m2f_grad_norm_finalize(const m2f_config* cfg, const double* scratch, const float* den_ptr, double max_norm, float* record,
                           m2f_stream_t stream);

/* Sharpness-aware minimisation (SAM; Foret et al., ICLR 2021) on the flat parameter buffer (optim.FusedAdam(sam_rho=...)).  No
 * counterpart in the reference.
 *
 * m2f_sam_perturb: w <- w + rho * g^ / (||g^|| + 1e-12), g^ = g / den (den = *grad_scale_ptr, or 1 when NULL), over every parameter
 * element.  `scratch` holds the partial sums of squares m2f_grad_sumsq has left for the SAME gradient buffer over ALL tensors.  Two
 * launches on `stream`: a finalize launch writes four floats, computed in float64 and rounded once each,
 *   record[0] = ||g^|| = sqrt(sum of squares) / den        record[1] = c = rho / (||g^|| + 1e-12) / den
 *   record[2] = den                                        record[3] = sqrt(sum of squares)
 * and the perturbation reads c when it runs: saved[i] <- params[i], params[i] <- fma(c, g[i], params[i]), one fused multiply-add per
 * element.  Exactly one of grads (fp32) / grads_bf16 (bf16, same indexing) is non-NULL; params, the gradients and saved (fp32, the
 * flat size) are 16-byte aligned.  param_shadow (the buffer of m2f_param_shadow_init, or NULL): the kernel also writes the W / W^T
 * bf16 shadows of every 2-D parameter from the perturbed value, as m2f_adam_step_shadowed lays them out.  The alignment pads between
 * tensors are neither read nor written in any buffer.  A zero gradient leaves every parameter's bits.  Same bits on every run.
 *
 * m2f_sam_restore: params[i] <- saved[i] over every parameter element (pads untouched): the bits from before the perturbation.  The
 * shadows are NOT rewritten: the caller's next optimizer step (or its casts) does that. */
int m2f_sam_perturb(const m2f_config* cfg, float* params, const float* grads, const uint16_t* grads_bf16, float* saved,
                    uint16_t* param_shadow, const double* scratch, const float* grad_scale_ptr, double rho, float* record,
                    m2f_stream_t stream);
int m2f_sam_restore(const m2f_config* cfg, float* params, const float* saved, m2f_stream_t stream);

/* Adversarial training on the input embeddings (FGM, Miyato et al. 2017; PGD, Madry et al. 2018; FreeLB, Zhu et al. 2020): the ascent
 * step on a perturbation delta of T token rows of width d (row stride ld: a multiple of 4 floats, >= d rounded up to 4; every buffer
 * 16-byte aligned).  No counterpart in the reference.  With (epsilon, step) = hyper_dev[0 .. 1] read ON THE DEVICE and ||.|| the L2 norm
 * of the row (norm_kind 0, "utterance") or over all rows that are not skipped (1, "batch"):
 *   u      = g / ||g||
 *   cand   = delta + step * u                      (||g|| == 0 or not finite: cand = delta)
 *   delta' = cand * min(1, epsilon / ||cand||)     (||cand|| == 0: delta' = cand)
 *   x      = x_clean + delta'                      (one fp32 add)
 * delta is updated in place.  key_pad (uint8 [T]): a row with a non-zero flag is neither read for a norm nor written - its x and delta
 * keep their bits; columns d .. ld - 1 are never written and enter no sum.  g NULL: a zero gradient (the projection alone).  The sums of
 * squares are float64 in one fixed order, the two quotients are rounded once to fp32, the elements are fp32 (cand = fma(step / ||g||, g,
 * delta)): ||delta'|| <= epsilon * (1 + 2^-22).  norm_kind 0: one launch, one wave per row, the row in registers for d <= 1,024 (a looping
 * form above).  norm_kind 1: two launches - float64 partials of sum g^2, sum delta^2 and sum delta . g per slice of 16 rows into
 * `scratch` (m2f_adv_scratch_bytes bytes, 16-byte aligned), then every workgroup adds them in index order and gets ||cand||^2 = sum delta^2 +
 * 2 (step / ||g||) sum delta . g + step^2 by algebra.  No atomics: same bits on every run.
 * m2f_adv_init: delta[t, c] = fp32(init_mag / sqrt(d)) * (2 * (h >> 8) * 2^-24 - 1) over the rows that are not skipped, h the dropout
 * hash (csrc/common.h: the hash behind the keep decision) of element t * d + c under `site` and the state rng_state (4 x uint32 on the
 * device); the other rows keep their bits. */
int64_t m2f_adv_scratch_bytes(int T);
int m2f_adv_ascend(int T, int d, int ld, const float* x_clean, const float* g, float* delta, float* x, const uint8_t* key_pad,
                   const float* hyper_dev, int norm_kind, void* scratch, m2f_stream_t stream);
int m2f_adv_init(int T, int d, int ld, float* delta, const uint8_t* key_pad, float init_mag, const uint32_t* rng_state, uint32_t site,
                 m2f_stream_t stream);

/* Per-tensor statistics and histograms of one flat buffer in the model's parameter layout (the model watch: what
 * wandb.watch(model, log="all") of the reference's loop, src/train.py:132-138, logs per parameter and per gradient tensor, computed
 * where the values live).  `a`: fp32, or (a_is_bf16 != 0) bf16 with the same indexing, 16-byte aligned; `b` (fp32, or NULL): the
 * statistics are those of x = a - b, one fp32 subtraction per element (a fp32).  Only parameter elements are read: the alignment
 * pads between tensors may hold anything.
 *
 * Three launches on `stream`: pass 1 (one partial per slice of 8192 elements of one tensor, into `scratch`), a finalize launch, and
 * pass 2, the histogram, a second read of the buffer.  record (m2f_tensor_stats_record_bytes(cfg, bins) bytes, 8-byte aligned, contents
 * irrelevant before the call):
 *   double[0] den = *den_ptr, or 1 when den_ptr is NULL   [1] number of tensors   [2] bins   [3] 0
 *   then one row per parameter tensor, in parameter-map order (m2f_param_layout):
 *     double[9]: numel, finite, nan, inf, zeros (x == 0), min, max over the finite values, their sum and sum of squares (float64
 *                accumulation); a tensor with no finite value has NaN in the last four
 *     int64[bins]: the counts of torch.histc(x[isfinite], bins, min, max) - pos = (int)((x - lo) * bins / (hi - lo)) in IEEE fp32 in
 *                that order, pos == bins counted in the last bin; lo, hi = min, max (lo - 1, hi + 1 when they are equal); all zero for
 *                a tensor with no finite value.
 * bins in [2, 256].  grid: workgroups of the two passes, <= 0 = default (at most 2048); nontemporal != 0: nontemporal loads.  Neither
 * changes a byte of the record, and two calls on the same buffer give the same bytes (float64 sums in a fixed order, integer counts).
 * m2f_tensor_stats_passes: the same with passes = 1 (pass 1 + finalize), 2 (pass 2 alone, onto the rows an earlier pass 1 left; it
 * ADDS its counts) or 3 (everything) - for timing the passes separately.  The size functions return -1 on a NULL configuration or bins
 * out of range. */
int64_t m2f_tensor_stats_scratch_bytes(const m2f_config* cfg, int bins);
int64_t m2f_tensor_stats_record_bytes(const m2f_config* cfg, int bins);
int m2f_tensor_stats(const m2f_config* cfg, const void* a, int a_is_bf16, const float* b, int bins, const float* den_ptr, void* scratch,
                     void* record, int grid, int nontemporal, m2f_stream_t stream);
int m2f_tensor_stats_passes(const m2f_config* cfg, const void* a, int a_is_bf16, const float* b, int bins, const float* den_ptr,
                            void* scratch, void* record, int grid, int nontemporal, int passes, m2f_stream_t stream);

/* Scoring of validation / test batches on the device: what the reference's loops do per batch on the host with torch and sklearn
 * (validate: src/train.py:245-272 - criterion(...).item(), argmax, the label != -1 masks, accuracy_score and
 * f1_score(average="weighted") per batch, averaged unweighted over the batches; test: src/test.py:51-74, the same without the loss).
 *
 * The rule, over the rows of one batch whose label is not -1: prediction = index of the first maximal logit (a NaN counts as
 * maximal, torch.argmax); cm[true][predicted] in integers; accuracy = trace / n; weighted F1 = (sum over c = 0 .. C-1 of
 * f_c * support_c) / n with f_c = 2 cm[c][c] / (support_c + predicted_c), 0 when that denominator is 0 (sklearn's default), both
 * in float64; loss = the criterion of m2f_loss / m2f_cross_entropy (num / den in fp32, the same bits for the same rows) without
 * its gradient.  A batch with no labelled row gives NaN three times.
 *
 * record (m2f_eval_record_bytes(C) bytes, 8-byte aligned, zeroed by the caller before a pass; every call ADDS one batch):
 *   double[0] loss_sum (the fp32 batch losses widened)  [1] acc_sum  [2] f1_sum  [3] n_batches
 *   double[4..6] loss, accuracy, weighted F1 of the LAST batch   [7] unused
 *   int64 [C][C] behind them: the confusion matrix of the whole pass.
 * scratch: m2f_eval_scratch_bytes(T, C) bytes, 8-byte aligned, contents irrelevant.  C <= 16.  Two launches, no atomics on
 * floats, no memset: capturable, and the same bytes on every run.
 *
 * m2f_eval_scores: logits [T, C] fp32 and labels [T] int64 of the caller, class_w [C] or NULL.
 * m2f_eval_step: the plan's forward (as m2f_forward: inputs from the staging buffers) followed by the scoring of M2F_BUF_LOGITS
 * against M2F_BUF_LABELS (class weights from M2F_BUF_CLASSW when use_class_weights), all T token rows of a padded or packed plan -
 * pad and filler rows carry label -1.  Eval plans and train plans without dropout; a train plan with dropout active is refused
 * (the reference validates under model.eval(), src/train.py:247).  use_graph = 1: the first call runs eagerly, later ones replay
 * one captured graph (re-captured when label_smoothing, use_class_weights, `record`, m2f_plan_params_fresh or the plan's launch
 * lists change).  Neither the flat gradient buffer, M2F_BUF_LOSS nor the dropout RNG state is touched. */
int64_t m2f_eval_scratch_bytes(int T, int C);
int64_t m2f_eval_record_bytes(int C);
int m2f_eval_scores(int T, int C, const float* logits, const int64_t* labels, const float* class_w, float label_smoothing,
                    void* scratch, void* record, m2f_stream_t stream);
int m2f_eval_step(m2f_plan* plan, float label_smoothing, int use_class_weights, void* record, int use_graph, m2f_stream_t stream);
/* m2f_eval_scores with the focal criterion's loss (m2f_plan_focal below: numerator (1 - p_y)^gamma * CE numerator, the bits of
 * m2f_cross_entropy_focal without a teacher for the same rows); gamma_dev: device float [1].  Confusion matrix, accuracy and weighted F1
 * do not depend on gamma.  m2f_eval_step runs this form while m2f_plan_focal(plan, 1) is on. */
int m2f_eval_scores_focal(int T, int C, const float* logits, const int64_t* labels, const float* class_w, float label_smoothing,
                          const float* gamma_dev, void* scratch, void* record, m2f_stream_t stream);

/* bf16-mode plans write every activation twice - fp32 and the bf16 shadow the GEMMs / attention kernels stage from.  When a plan
 * is built, the readers of every workspace buffer are enumerated from its final launch lists; a copy nobody reads is not written
 * (fp32 of QKV projections, attention outputs, their gradients and the FFN hidden gradients; the shadows of results that are only
 * residual terms or LayerNorm inputs), and its buffer is filled with NaNs once so
 * that an unknown reader cannot go unnoticed.  Returns how many copies this plan skips (0: fp32 mode, or M2F_SKIP_F32=0 when the
 * plan was built).  Results are bit-identical either way.  No counterpart in the reference (autocast keeps one copy per tensor). */
int m2f_plan_skipped_copies(m2f_plan* plan);

/* ---- in-loop text encoder (BASELINE config C5) -------------------------------------------------
 * The reference computes its text embeddings with transformers' RobertaModel (src/feature_extractors/text/model.py:16-21,
 * [CLS] pooling at text/embeddings.py:83) in a separate stage; these entry points are the pieces that model needs beyond
 * the GEMM / LayerNorm kernels below, so the encoder can run in the training loop on the same device buffers. */

/* Outputs of m2f_gemm / m2f_layernorm_fwd / m2f_embed_layernorm / m2f_attention_long_fwd that lie inside
 * [ws_base, ws_base + floats) are ALSO written as bf16 at the same element index of `shadow` (the operand copies the
 * bf16 GEMM stages from).  NULL, NULL, 0 switches it off.  Thread-local. */
int m2f_set_shadow_map(const float* ws_base, uint16_t* shadow, int64_t floats);

/* RobertaEmbeddings.forward in eval mode: out[t] = LayerNorm(word_emb[input_ids[t]] + pos_emb[position_ids[t]] +
 * token_type_emb[0]) for T tokens of width d (d % 4 == 0, d <= 2048). */
int m2f_embed_layernorm(int T, int d, const int64_t* input_ids, const int64_t* position_ids, const float* word_emb,
                        const float* pos_emb, const float* type_emb_row0, const float* gamma, const float* beta, float eps,
                        float* out, int ld_out, m2f_stream_t stream);

/* Token-level multi-head self-attention, forward only, any sequence length S (RobertaSelfAttention in eval mode):
 * q/k/v rows are tokens t = b*S + i, head h in columns [h*hd, (h+1)*hd), hd <= 128; key_pad [B, S] (1 = padded key,
 * nullable); softmax(q k^T / sqrt(hd) + mask) v with an online softmax over 64-key blocks. */
int m2f_attention_long_fwd(int B, int S, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                           const uint8_t* key_pad, float* out, int ldo, m2f_stream_t stream);

/* The same attention on bf16 operands (round 4; the encoder's bf16 mode): q / k / v are the bf16 result of the packed projection
 * GEMM as it is (leading dimensions in elements; hd, the leading dimensions and the addresses multiples of 8 elements), the products run on
 * v_mfma_f32_16x16x16_bf16 with fp32 accumulation and an fp32 online softmax, probabilities rounded to bf16 for the P V product (the
 * denominator sums the rounded values); out16 (bf16) is always written, out32 (fp32, same indexing) when not NULL.  hd <= 128. */
int m2f_attention_long_fwd_bf16(int B, int S, int H, int hd, const uint16_t* q, int ldq, const uint16_t* k, int ldk, const uint16_t* v,
                                int ldv, const uint8_t* key_pad, uint16_t* out16, float* out32, int ldo, m2f_stream_t stream);

/* ... with a third output (nullable like the others; at least one must be given): out8 = OCP e4m3 bytes of value * out8_scale,
 * saturating at +-448 - the operand the fp8 output projection stages (no fp32 copy, no quantise pass); needs hd and ldo in multiples of 16. */
int m2f_attention_long_fwd_bf16_out8(int B, int S, int H, int hd, const uint16_t* q, int ldq, const uint16_t* k, int ldk,
                                     const uint16_t* v, int ldv, const uint8_t* key_pad, uint16_t* out16, float* out32, uint8_t* out8,
                                     float out8_scale, int ldo, m2f_stream_t stream);

/* Diagnostic (tools/ln_stats_ab.py): one LayerNorm-forward launch over 1..4 problems of T rows, as the plans merge them; pre = 1 reads
 * (mean, rstd) from `stats` instead of computing them - the cost of a LayerNorm whose statistics came out of the preceding GEMM's epilogue. */
int m2f_layernorm_fwd_diag(int T, int n_prob, const int* d, const float* const* x, const float* const* gamma, const float* const* beta, float* const* out,
                           float* const* stats, float eps, int pre, m2f_stream_t stream);

/* m2f_layernorm_fwd that ALSO writes its result as e4m3(value * out8_scale), saturating, into out8 [T, d] (d % 4 == 0): the fp8 text
 * encoder's LayerNorm outputs are GEMM operands (round 4: replaces a quantise pass over the fp32 result). */
int m2f_layernorm_fwd_out8(int T, int d, const float* x, const float* gamma, const float* beta, const float* res, float* out,
                           float* stats, float eps, uint8_t* out8, float out8_scale, m2f_stream_t stream);

/* Results of the following m2f_gemm calls of this thread that have a bf16 shadow (m2f_set_shadow_map) have NO fp32 reader: kernels
 * that know how (the chip-filling bf16 forms) write the shadow only and leave the fp32 buffer untouched; edge tiles and the other
 * forms still write both.  0 switches it off.  (The plans decide this per buffer from their launch lists: m2f_plan_skipped_copies.) */
int m2f_set_shadow_only(int on);

/* fp8 GEMM of the in-loop text encoder (BASELINE C5 asks for fp8 MFMA): C[M,N] = act(acc_scale * A8 B8^T + bias) + res with
 * A8 [M,K], B8 [N,K] row-major OCP e4m3 bytes (K, lda, ldb multiples of 16; 16-byte aligned), fp32 accumulate on
 * v_mfma_f32_32x32x16_fp8_fp8; acc_scale = 1 / (scale_a * scale_b) undoes the per-tensor quantisation scales.
 * activation: 0 none, 1 ReLU, 2 GELU.  c8 (nullable): the result is written as e4m3(result * c8_scale) at c8[m*ldc + n]
 * INSTEAD of fp32 c (an activation whose only reader is the next fp8 GEMM, e.g. the FFN hidden layer).  Forward only. */
int m2f_gemm_fp8(int M, int N, int K, const uint8_t* a8, int lda, const uint8_t* b8, int ldb, float acc_scale, float* c, int ldc,
                 const float* bias, const float* res, int ldres, int activation, uint8_t* c8, float c8_scale,
                 m2f_stream_t stream);

/* dst[i] = e4m3(clamp(src[i] * scale, +-448)), n % 4 == 0: operand quantisation for m2f_gemm_fp8. */
int m2f_quantize_fp8(const float* src, uint8_t* dst, int64_t n, float scale, m2f_stream_t stream);

/* ---- kernel-level entry points (used by the parity tests; same kernels the plan launches) ---------- */
/* Number of bf16 GEMM launches this process has issued in the RING form (csrc/gemm_ring.h, m2f_gemm16_ring_kernel: LDS-direct
 * operand ring; taken by k-contiguous launches of at least M2F_RING_MIN = 200 tiles of 128x128 unless M2F_RING=0; DESIGN.md, "GEMM
 * dispatch") or the eight-phase form.  Diagnostic: lets a test assert that the form it means to check actually ran. */
long long m2f_gemm_ring_launches(void);
/* The kernel form the last m2f_gemm / m2f_gemm_fp8 / m2f_gemm_p8 call (or any GEMM launch of a plan) dispatched to: one
 * M2F_FORM_* value, plus M2F_FORM_VEC when the fp32-source or skinny kernel moves its operands in 16-byte chunks, M2F_FORM_SRC16
 * when the skinny kernel reads bf16 shadows, and M2F_FORM_NN_T when a bf16 NN launch ran as the k-contiguous form through the
 * transposed shadows; M2F_FORM_NONE after a call that launched nothing.  Host-side diagnostic: lets a test assert the kernel it covers.
 * Assigned at ONE site for every dispatched launch - execute() in csrc/gemm_dispatch.hip, from the chooser's GemmChoice::form; the
 * direct entry m2f_gemm_p8 and the table launches (csrc/gemm_p8.hip), which do not go through the chooser, assign their own. */
int m2f_gemm_last_form(void);
enum {
    M2F_FORM_NONE = 0,
    M2F_FORM_F32SRC_64 = 1,            /* m2f_gemm_kernel: fp32 mode, or bf16 mode staged from fp32 originals; 64x64 tiles */
    M2F_FORM_F32SRC_128 = 2,           /* ... 128x128 tiles */
    M2F_FORM_F32SRC_SPLITK = 3,        /* ... 64x64 tiles, in-launch split-K */
    M2F_FORM_BF16SRC_64 = 4,           /* m2f_gemm16_kernel: register-staged from bf16 shadows; 64x64 tiles */
    M2F_FORM_BF16SRC_128 = 5,          /* ... 128x128 tiles */
    M2F_FORM_BF16SRC_256x128 = 6,      /* ... 256x128 tiles */
    M2F_FORM_RING_64x64 = 7,           /* m2f_gemm16_ring_kernel, gemm_ring.h */
    M2F_FORM_RING_128x64 = 8,
    M2F_FORM_RING_128x128 = 9,
    M2F_FORM_RING_256x128 = 10,
    M2F_FORM_P8_KC = 11,               /* eight-phase 256x256 form, gemm_p8.h: k-contiguous operands */
    M2F_FORM_P8_RC = 12,               /* ... row-major (weight-gradient) operands, table launch */
    M2F_FORM_SKINNY_NT = 13,           /* skinny.hip: the classifier head */
    M2F_FORM_SKINNY_NN = 14,
    M2F_FORM_FP8_128x128 = 15,         /* register-staged e4m3 form */
    M2F_FORM_FP8_256x128 = 16,
    M2F_FORM_FP8_RING = 17,            /* ring form, 256x128 tiles, e4m3 operands */
    M2F_FORM_FP8_P8 = 18,              /* eight-phase form, e4m3 operands */
    M2F_FORM_VEC = 0x100,
    M2F_FORM_SRC16 = 0x200,
    M2F_FORM_NN_T = 0x400
};

/* Dry run of the GEMM dispatch (host only, no HIP call, works without a GPU): the M2F_FORM_* value - bits included - that m2f_gemm
 * (mode 0 = fp32, 1 = bf16) or m2f_gemm_fp8 (mode 2; layout 0, K1 = 0) would record for `count` (1 .. 8, one launch) identical problems
 * of M x N x (K0 + K1) under the forced `tile` (0 = automatic); M2F_FORM_NONE for a launch the entry refuses.  It asks the chooser the
 * launchers ask (csrc/gemm_dispatch.hip) on a synthetic batch: aligned operands that are never dereferenced, every leading dimension
 * pad8 of its contiguous extent.  bits: what the dispatch rules look at.  stages_bf16 (nullable; modes 0 / 1): 1 when a bf16-mode
 * launch of the batch reads bf16 shadows only (what the plan's unread-copy analysis asks). */
enum {
    M2F_GEMM_FORM_SHADOWS = 1,         /* every operand segment has a bf16 shadow */
    M2F_GEMM_FORM_BT_SHADOW = 2,       /* ... and B a transposed one (layout 1) */
    M2F_GEMM_FORM_ODD_LD = 4,          /* leading dimensions pad8(extent) + 1: neither 16-byte loads nor shadow staging */
    M2F_GEMM_FORM_BIAS_GRAD = 8,
    M2F_GEMM_FORM_GELU = 16,
    M2F_GEMM_FORM_RELU_B = 32,
    M2F_GEMM_FORM_ACC = 64,
    M2F_GEMM_FORM_GATE = 128,
    M2F_GEMM_FORM_DROP = 256,          /* a dropout site in the epilogue */
    M2F_GEMM_FORM_C8 = 512,            /* fp8: the result leaves as e4m3 */
    M2F_GEMM_FORM_SPLITK = 1024,       /* split-K scratch present */
    M2F_GEMM_FORM_RELU_A = 2048,
    M2F_GEMM_FORM_RELU_OUT = 4096,
    M2F_GEMM_FORM_RES = 8192
};
int m2f_gemm_form(int mode, int layout, int tile, int count, int M, int N, int K0, int K1, uint32_t bits, int* stages_bf16);

/* C[M,N] = epilogue(A x B); layout 0: C = A[M,K] B[N,K]^T (nn.Linear forward), 1: C = A[M,K] B[K,N]
 * (input gradient), 2: C = A[K,M]^T B[K,N] (weight gradient; bias_grad[M] = column sums of A; with accumulate != 0 both C and
 * bias_grad accumulate: bias_grad[M] += the column sums).
 * Optional second operand segment (a1/b1, k1) = never-materialised torch.cat along the reduction dim. */
int m2f_gemm(int precision, int layout, int M, int N, int K0, int K1,
             const float* a0, int lda0, const float* a1, int lda1,
             const float* b0, int ldb0, const float* b1, int ldb1,
             float* c, int ldc, const float* bias, const float* res, int ldres,
             const float* gate, int ldgate, float gate_scale, float* bias_grad,
             int relu_a, int relu_b, int relu_out /* 0 none, 1 ReLU, 2 exact GELU */, int accumulate,
             uint32_t drop_site, float drop_p, const uint32_t* rng_state, int tile,
             float* splitk_ws, uint32_t* splitk_tickets, int splitk_max_tiles,
             const uint16_t* a0_bf16, int lda0_bf16, const uint16_t* a1_bf16, int lda1_bf16,
             const uint16_t* b0_bf16, int ldb0_bf16, const uint16_t* b1_bf16, int ldb1_bf16, m2f_stream_t stream);
/* a*_bf16 / b*_bf16 (nullable): bf16 copies of the operands (same logical elements; leading dimensions multiples of 8,
 * pad columns zero).  In bf16 mode a launch whose operands all have one stages from them (half the bytes per CU).
 * splitk_ws / splitk_tickets (nullable): scratch for in-launch split-K of launches too small to fill the chip:
 * splitk_max_tiles * 4 * 64*64 floats and splitk_max_tiles ZEROED uint32 tickets (re-armed by the kernel). */
/* ---- optimizer inside the step (round 4) ----------------------------------------------------------------------
 * torch.optim.Adam.step (src/train.py:56,231) applied where the weight gradient is born: the weight-gradient launch of a bf16 train
 * plan (eight-phase table form, M2F_TABLE_TILE=132) updates p / exp_avg / exp_avg_sq and both bf16 parameter shadows of the elements
 * whose dW it holds in registers, and one launch of the shadow-writing Adam kernel updates everything else (biases, LayerNorm, the
 * few matrices outside the table) - all inside m2f_step's captured graph.  dW of the table's matrices is NOT written to `grads`.
 * Same arithmetic as m2f_adam_step_shadowed on the same gradients: bit-identical parameters, moments and shadows.
 * setup: buffers as for m2f_adam_step_shadowed (params = the plan's parameter buffer, param_shadow = the buffer the plan was created
 * with); hyper_dev = 8 device floats refreshed by m2f_adam_hyper BEFORE every step (lr, betas, eps, weight decay, step count t >= 1:
 * lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) change every step and a replayed graph cannot take them as arguments);
 * grad_scale_ptr (nullable): device scalar the gradients are divided by (m2f_step(normalise = 0)).
 * m2f_plan_fused_adam(plan, 1 | 0) switches the form of the NEXT m2f_step (re-captures the graph on a change, and after every setup). */
int m2f_plan_fused_adam_setup(m2f_plan* plan, float* params, float* exp_avg, float* exp_avg_sq, uint16_t* param_shadow,
                              const float* hyper_dev, const float* grad_scale_ptr);
int m2f_plan_fused_adam(m2f_plan* plan, int on);
int m2f_adam_hyper(float* hyper_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int step, m2f_stream_t stream);

/* ---- parameter groups and decoupled weight decay ---------------------------------------------------------------
 * optimizer.step() of torch.optim.Adam / torch.optim.AdamW built over SEVERAL param_groups, or over a subset of the model's parameters
 * (the reference's stage-1 trainers: feature_extractors/text/train.py:62-63, audio_wav2vec2/train.py:62-63 - torch.optim.AdamW over the
 * head alone, then over everything), each group with its own lr / betas / eps / weight_decay and step count.
 *
 * m2f_adam_hyper_groups: refreshes the hyper table - n_groups <= M2F_ADAM_MAX_GROUPS rows of 8 floats in device memory (lr / bc1, beta1,
 * beta2, eps, coupled weight decay, 1 / sqrt(bc2), decay, spare) - from `groups`, one small launch on `stream`, the values passed by
 * value (no host sync; `groups` may be freed at once).  decoupled != 0 (AdamW): decay = 1 - lr * weight_decay, formed in double and
 * rounded once as torch forms the scalar of param.mul_, and the coupled weight decay of the row is 0; otherwise decay = 1 and the row
 * is torch.optim.Adam's.  step >= 1 is the group's own count (bias corrections).  Kernels read the table when they run, so a captured
 * graph that holds them follows a scheduler's new lr without a re-capture.
 *
 * m2f_adam_step_grouped: the update of the tensors at flat offsets [first, end) (both the offset of a parameter tensor; end < 0: to the
 * last one) that some group owns.  tensor_group: n_tensors host ints in parameter order (m2f_param_layout), the group of each tensor
 * or -1 = owned by none: such a tensor, its moments and its shadows are neither read nor written.  param_shadow non-NULL (bf16 mode,
 * the buffer of m2f_param_shadow_init): the kernel also writes W / W^T shadows of what it updates, as m2f_adam_step_shadowed_range does;
 * NULL (fp32 mode): slices of at most 8192 elements of one tensor each, the alignment pads between tensors are not touched.
 * A group whose row is Adam's gives m2f_adam_step / m2f_adam_step_shadowed's bits on its tensors.  Device copies of the item / slice
 * lists are cached per (configuration, device, map). */
#define M2F_ADAM_MAX_GROUPS 16
typedef struct m2f_adam_group {
    double lr;                                 /* torch keeps it as a double; lr / bc1 is formed from (float)lr as m2f_adam_step does */
    float beta1, beta2, eps, weight_decay;
    int decoupled;                             /* 0: torch.optim.Adam (coupled L2), 1: torch.optim.AdamW */
    int step;                                  /* >= 1 */
} m2f_adam_group;
int m2f_adam_hyper_groups(float* hyper_table, const m2f_adam_group* groups, int n_groups, m2f_stream_t stream);
int m2f_adam_step_grouped(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg, float* exp_avg_sq,
                          uint16_t* param_shadow, const int* tensor_group, int n_tensors, const float* hyper_table, int64_t first,
                          int64_t end, const float* grad_scale_ptr, m2f_stream_t stream);
/* Exponential moving average (EMA) of the weights inside the optimizer kernels (optim.FusedAdam(ema_decay=...)).  Replaces
 * torch.optim.swa_utils.AveragedModel.update_parameters with multi_avg_fn = get_ema_multi_avg_fn(decay) called after optimizer.step():
 * the kernel that has the updated parameter in registers also reads, updates and writes its average - 8 B per parameter on top of the
 * update's own traffic instead of a second pass of 12 B, and one launch fewer.  No counterpart in the reference, whose loop scores the
 * live weights.  `ema`: fp32, indexed and 16-byte aligned like `params`; ema_w = (float)(1 - decay) with 1 - decay formed in double, in
 * [0, 1], ONE value for every launch of a step and every group:
 *   e <- (ema_w == 1) ? p_new : fma(ema_w, p_new - e, e)
 * ema_w == 1 is the first update, torch's n_averaged == 0 copy: the average takes the parameter's bits whatever the buffer held.
 * Parameters, moments and shadows get the bits of the entry point without the suffix; every form gives the average the same bits.
 *
 * m2f_adam_step_ema / m2f_adam_step_g16_ema: m2f_adam_step / m2f_adam_step_g16 with the average over the same n elements (pads between
 * tensors included: a zero parameter pad keeps a zero average).
 * m2f_adam_step_shadowed_range_ema: m2f_adam_step_shadowed_range with the average of the tensors of [first, end).
 * m2f_adam_step_grouped_ema: m2f_adam_step_grouped with the average of the OWNED tensors of [first, end); the EMA slice of a tensor
 * no group owns is neither read nor written. */
int m2f_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int step, float ema_w, const float* grad_scale_ptr, m2f_stream_t stream);
int m2f_adam_step_g16_ema(float* params, const uint16_t* grads_bf16, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float ema_w, const float* grad_scale_ptr,
                          m2f_stream_t stream);
int m2f_adam_step_shadowed_range_ema(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg,
                                     float* exp_avg_sq, uint16_t* param_shadow, float* ema, float ema_w, int64_t first, int64_t end,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                     const float* grad_scale_ptr, m2f_stream_t stream);
int m2f_adam_step_grouped_ema(const m2f_config* cfg, float* params, const void* grads, int grads_bf16, float* exp_avg, float* exp_avg_sq,
                              uint16_t* param_shadow, float* ema, float ema_w, const int* tensor_group, int n_tensors,
                              const float* hyper_table, int64_t first, int64_t end, const float* grad_scale_ptr, m2f_stream_t stream);
/* m2f_ema_exchange: params[i] <-> ema[i] in place over every element of the tensors a group owns (tensor_group as in
 * m2f_adam_step_grouped; all >= 0: every tensor) - evaluating with the averaged weights (what scoring AveragedModel.module instead of
 * the model is in torch) without a copy through the host or a third buffer.  The alignment pads and the tensors of no group are not
 * touched; a second call restores both buffers bit for bit.  The caller re-casts the bf16 parameter shadows afterwards. */
int m2f_ema_exchange(const m2f_config* cfg, float* params, float* ema, const int* tensor_group, int n_tensors, m2f_stream_t stream);

/* m2f_plan_fused_adam_setup for a grouped optimizer (torch.optim.AdamW(groups).step inside m2f_step): hyper_table = the rows of
 * m2f_adam_hyper_groups (refreshed BEFORE every step), tensor_group as above.  The weight-gradient launch updates a matrix with the row
 * of its group; the residual launch is the grouped shadow-writing kernel over the owned tensors the table does not cover.  Fails when a
 * matrix of the weight-gradient table is owned by no group (its gradient would have nowhere to go: the caller takes the two-launch path).
 * Drops the plan's captured step, as every setup does; m2f_plan_fused_adam(plan, 1 | 0) switches the form as before. */
int m2f_plan_fused_adam_setup_grouped(m2f_plan* plan, float* params, float* exp_avg, float* exp_avg_sq, uint16_t* param_shadow,
                                      const float* hyper_table, const int* tensor_group, int n_tensors, const float* grad_scale_ptr);

/* Gradients left as bf16 (round 4; the data-parallel bf16 exchange, multimodal-emotion-recognition_amd/dp.py): after m2f_plan_grad_bf16(plan, g16)
 * a step writes EVERY gradient, rounded once to bf16, at its element index of g16 (n_params uint16, 16-byte aligned) - the weight
 * gradients of the table launch directly (no fp32 dW: -2 bytes per parameter written, and no rounding pass over the fp32 buffer before
 * the all-reduce), all others through one cast launch behind the backward.  The fp32 buffer then holds only those others (and the loss
 * tail).  m2f_plan_grad_bf16(plan, NULL) restores fp32 gradients.  Same bits as rounding the fp32 gradients of a plain step. */
int m2f_plan_grad_bf16(m2f_plan* plan, uint16_t* grads_bf16);

/* Gradient accumulation over micro-batches: while m2f_plan_accumulate_grads(plan, 1) is on, m2f_backward / m2f_step of the plan ADD
 * every parameter gradient into `grads` (old + new, one rounded fp32 add of the value the overwrite form stores: the sum of two
 * backwards equals the fp32 sum of their overwrite-form gradients bit for bit), and m2f_loss / m2f_step add den and num of the
 * criterion tail (grads[n_params + 1], grads[n_params + 2]) to what it holds; grads[n_params] is still this batch's num / den.  The
 * caller zeroes what starts a group.  Plans that share one gradient buffer accumulate into it together.  The accumulate launch lists
 * and the step graph of that form are built the first time it is switched on (a plan that never accumulates keeps its lists and graph);
 * m2f_plan_accumulate_grads(plan, 0) restores the overwrite form.  Fails for a plan without a gradient buffer, with fused Adam on or
 * bf16 gradients armed; while it is on, m2f_step_part, m2f_plan_fused_adam(plan, 1) and m2f_plan_grad_bf16(plan, non-NULL) fail. */
int m2f_plan_accumulate_grads(m2f_plan* plan, int on);

/* The adversarial state of a train plan: per modality of modality_mask (1 text, 2 audio; enabled modalities only) a perturbation
 * delta and a copy x_clean of the staged input, [T, pad8(d)] floats each, beside (epsilon, step_size), the rows' skip flags and the
 * batch norm's scratch - all inside `state`, the CALLER's device buffer of m2f_plan_adversarial_bytes bytes (256-byte aligned, kept
 * alive while it is on; as m2f_plan_stream_speakers takes its buffer): a plan that never asks has the workspace it always had.  The ids
 * M2F_BUF_ADV .. M2F_BUF_ADV_DELTA_AUDIO then point into it.  modality_mask 0 (or state NULL): off.  Nothing here changes a launch list
 * or a captured graph: the ascent writes the fp32 staging buffers M2F_BUF_TEXT / M2F_BUF_AUDIO, which every forward reads (in bf16 mode
 * through the input casts at the head of its launch list).
 * m2f_plan_adv_begin: x_clean <- the staged inputs, delta <- 0 (device-to-device copies and fills on `stream`); init_mag > 0: delta <-
 * the uniform start of m2f_adv_init under M2F_ADV_SITE_TEXT / M2F_ADV_SITE_AUDIO and the plan's dropout state as it is now (NULL state:
 * refused), projected onto the epsilon ball of norm_kind, and the staged inputs <- x_clean + delta.  The caller has written
 * M2F_BUF_ADV_SKIP and M2F_BUF_ADV on the stream before.
 * m2f_plan_adv_ascend: m2f_adv_ascend per modality on the plan's own M2F_BUF_DTEXT / M2F_BUF_DAUDIO (the plan computes them:
 * m2f_plan_backward_outputs with the modality's bit), delta and x_clean, writing the staged inputs.  One launch per norm_kind-0 call and
 * modality, two per norm_kind-1 call; waits for nothing. */
int64_t m2f_plan_adversarial_bytes(m2f_plan* plan, int modality_mask);
int m2f_plan_adversarial(m2f_plan* plan, int modality_mask, void* state, int64_t state_bytes);
int m2f_plan_adv_begin(m2f_plan* plan, float init_mag, int norm_kind, m2f_stream_t stream);
int m2f_plan_adv_ascend(m2f_plan* plan, int norm_kind, m2f_stream_t stream);

/* Distillation criterion: while m2f_plan_distill(plan, 1) is on, the criterion launch of m2f_loss / m2f_step / m2f_step_part /
 * m2f_step_timed blends the hard-label cross entropy with the KL divergence from a teacher's logits (M2F_BUF_TEACHER), per token row
 * (z the plan's logits, u the teacher's, q = softmax(z / tau), p = softmax(u / tau), w_y the class weight of the label or 1):
 *   num = (1 - alpha) * numCE + alpha * tau^2 * w_y * sum_c p_c (log p_c - log q_c)        den = w_y (unchanged)
 *   dlogits = (1 - alpha) * dCE + alpha * tau * w_y * (q - p)                              (unnormalised, as ever)
 * and loss = sum num / sum den through the unchanged tail: ONE denominator, so normalise = 0, the accumulate form and the
 * data-parallel division by the global den hold as they are.  Without class weights this is (1 - alpha) * CrossEntropyLoss(...) +
 * alpha * tau^2 * kl_div(log_softmax(z / tau), softmax(u / tau), reduction='batchmean') over the labelled rows.  alpha = 0 gives
 * the plain criterion's bits.  Rows with label -1 (or out of range) write zeros whatever their teacher row holds.
 * alpha, tau = M2F_BUF_DISTILL[0], [1] are read ON THE DEVICE by every step (a captured step follows a schedule without a new
 * capture); the call itself writes nothing and waits for nothing: the caller writes its pair (tau > 0) and the teacher rows on its
 * stream before the first step, the teacher rows before each step.  A change of the switch bumps the plan's generation: no captured step replays the other criterion.  Works with fused
 * Adam, bf16 gradients and the accumulate form.  Fails for a plan without a gradient buffer. */
int m2f_plan_distill(m2f_plan* plan, int on);

/* Focal criterion (Lin et al. 2017): while m2f_plan_focal(plan, 1) is on, the criterion launch of m2f_loss / m2f_step / m2f_step_part /
 * m2f_step_timed and the rows launch of m2f_eval_step scale the hard-label term of every labelled token row by (1 - p_y)^gamma
 * (p = softmax(z), y the label, numCE / dCE the plain criterion's numerator and gradient, omp = sum of p_c over c != y):
 *   num = omp^gamma * numCE                                                                den = w_y (unchanged)
 *   dlogits_c = omp^gamma * dCE_c + numCE * gamma * omp^(gamma-1) * p_y * d_c              d_c = p_c (c != y), d_y = -omp
 * and loss = sum num / sum den through the unchanged tail.  Without class weights and smoothing this is the mean over the labelled rows
 * of -(1 - p_y)^gamma log p_y.  With m2f_plan_distill on as well the factor scales the hard-label term only:
 * num = (1 - alpha) * omp^gamma * numCE + alpha * tau^2 * w_y * KL; the teacher's gradient term is unchanged.
 * gamma = M2F_BUF_FOCAL[0], in [0, 8], is read ON THE DEVICE by every step (a captured step follows a schedule without a new capture);
 * the call writes nothing and waits for nothing: the caller writes gamma on its stream before the first step.  gamma = 0 gives the
 * bits of the criterion without the switch.  A row whose other classes' probabilities all underflow (omp = 0) contributes zero loss
 * and zero gradient for gamma > 0; no gamma produces a NaN from finite logits.  A change of the switch bumps the plan's generation: no
 * captured step or eval step replays the other form; a change of gamma alone does not.  Train and eval plans; works with fused Adam,
 * bf16 gradients, the accumulate form and distillation. */
int m2f_plan_focal(m2f_plan* plan, int on);

/* R-Drop criterion (Liang et al. 2021): while m2f_plan_rdrop(plan, 1) is on, the criterion launch of m2f_loss / m2f_step / m2f_step_part /
 * m2f_step_timed couples every token row r with its twin t(r) = M2F_BUF_PARTNER[r] - the same utterance a second time in the SAME plan,
 * which the hashed dropout streams give an independent mask at every site - and adds the symmetric KL divergence between the two
 * predictions (p = softmax(z_r), q = softmax(z_t(r)), y the shared label, numCE / dCE the plain criterion's numerator and gradient):
 *   s_r       = 0.5 * (KL(p || q) + KL(q || p))                                        (the same bits on both rows of a pair)
 *   num_r     = numCE_r + alpha * w_y * s_r                                            den_r = w_y (unchanged)
 *   dlogits_r = dCE_r + alpha * w_y * (p * ((log p - log q) - KL(p || q)) + (p - q))
 * and loss = sum num / sum den through the unchanged tail; the fourth float of the tail (loss_out[3]) receives sum w_y * s_r, the KL
 * share of the numerator WITHOUT alpha, summed in the tail's own fixed order (added to by the accumulate form, summed over ranks by the
 * all-reduce of the tail).  alpha = M2F_BUF_RDROP[0] >= 0 is read ON THE DEVICE by every step, and M2F_BUF_PARTNER is an input like
 * M2F_BUF_CU_SEQLENS: the call writes nothing and waits for nothing, the caller writes both on its stream before the first step.  A twin
 * index outside [0, T) means no twin: the plain term.  alpha = 0 gives the bits of the criterion without the switch; a row without a
 * valid label writes zeros whatever its twin holds.  A change of the switch bumps the plan's generation: no captured step replays the
 * other form; a change of alpha or of the map does not.  Train plans with a gradient buffer only (m2f_eval_step keeps the hard-label
 * criterion); works with fused Adam, bf16 gradients and the accumulate form.  Refused while m2f_plan_distill, m2f_plan_focal or
 * m2f_plan_crf is on, and each of them refuses while this is on. */
int m2f_plan_rdrop(m2f_plan* plan, int on);

/* Supervised contrastive criterion (Khosla et al. 2020) on the classifier's last hidden activation: while m2f_plan_supcon(plan, 1) is on,
 * the criterion of m2f_loss / m2f_step / m2f_step_part / m2f_step_timed is the plan's cross entropy PLUS, per token row,
 *   num_i += lambda * w_{y_i} * l_i                                            den_i = w_{y_i} (unchanged: one denominator)
 * over h_i = row i of M2F_BUF_FEATURES (post-ReLU, post-dropout in train mode), with the definition of m2f_supcon below: V = the rows with
 * a label in [0, C) and ||h_i|| > 0, z_i = h_i / ||h_i||, s_ia = z_i . z_a / tau, A(i) = V \ {i}, P(i) = {a in A(i): y_a = y_i}, n_i = |P(i)|,
 * l_i = lse_{a in A(i)} s_ia - (1 / n_i) sum_{p in P(i)} s_ip for n_i > 0, else 0.  The contrast set is the WHOLE plan: every dialogue of the
 * batch, in whatever token rows the plan keeps them.  The gradient dh_i (m2f_supcon's dfeatures), scaled by what the finalize launch scales
 * dlogits by (1 / den with normalise, the same bits; 1 without), enters the backward behind the GEMM that produces the gradient of that
 * activation: dh[i, :] += (h[i, :] > 0 ? gate_scale : 0) * dh_i, one launch that also rewrites dh's bf16 shadow in bf16 mode.  The fourth
 * float of the tail (loss_out[3]) receives sum w_{y_i} l_i WITHOUT lambda, in the tail's own fixed order (added to by the accumulate form).
 * (lambda, tau) = M2F_BUF_SUPCON[0 .. 1], lambda >= 0 and tau > 0, are read ON THE DEVICE by every step: the call writes nothing and waits for
 * nothing, the caller writes them on its stream before the first step.  lambda = 0 gives the loss and the gradients of the criterion without
 * the switch.  The kernels run in exact fp32 in both precision modes.  A change of the switch bumps the plan's generation: no captured step
 * replays the other form; a change of lambda or tau does not.  Train plans with a gradient buffer only (m2f_eval_step keeps the hard-label
 * criterion); works with fused Adam, bf16 gradients and the accumulate form (each micro-batch contrasts within itself).  Refused while
 * m2f_plan_distill, m2f_plan_focal, m2f_plan_rdrop or m2f_plan_crf is on, and each of them refuses while this is on. */
int m2f_plan_supcon(m2f_plan* plan, int on);

/* Auxiliary label head (a second linear classifier over the classifier's last hidden activation, scored against a second label per token
 * row; the kernel-level entry m2f_aux_head below defines it): while m2f_plan_aux_head(plan, params, param_grad, num_aux) is on, the
 * criterion of m2f_loss / m2f_step / m2f_step_part / m2f_step_timed is the plan's cross entropy (plain or focal) PLUS, per token row with
 * a label y_i in [0, C) AND an auxiliary label s_i = M2F_BUF_AUX_LABELS[i] in [0, num_aux),
 *   u_i = W h_i + b,   a_i = label-smoothed CE(u_i, s_i; eps_a),   num_i += lambda * w_{y_i} * a_i        den_i = w_{y_i} (unchanged)
 * over h_i = row i of M2F_BUF_FEATURES (post-ReLU, post-dropout in train mode).  u goes to M2F_BUF_AUX_LOGITS.  The gradient enters the
 * backward behind the GEMM that produces the gradient of that activation: dh[i, :] += (h[i, :] > 0 ? gate_scale : 0) * scale * lambda *
 * sum_c g[i, c] W[c, :] with g = w_y d a / d u and scale what the finalize launch scales dlogits by (1 / den with normalise, the same
 * bits; 1 without) - one launch that also rewrites dh's bf16 shadow in bf16 mode.  The fourth float of the tail (loss_out[3]) receives
 * sum w_{y_i} a_i WITHOUT lambda, in the tail's own fixed order (added to by the accumulate form).
 * params: device float [num_aux * cls_hidden + num_aux] = [W row-major | b], 16-byte aligned, 2 <= num_aux <= 16, the CALLER's (as
 * m2f_plan_crf's block): not in the flat parameter buffer, m2f_config or any optimizer table; its VALUES are read on the device at every
 * step.  param_grad: device float of the same size, OVERWRITTEN by every step with scale * lambda * [g^T h | sum_i g_i]; NULL: the head
 * is frozen, a pure input.  params NULL: off.  (lambda, eps_a) = M2F_BUF_AUX[0 .. 1], lambda >= 0 and 0 <= eps_a < 1, are read ON THE
 * DEVICE by every step; lambda = 0 gives the loss and the gradients of the criterion without the switch.  Exact fp32 in both precision
 * modes.  A change of the pointers, the switch or num_aux bumps the plan's generation; a change of the values does not.  Train plans
 * with a gradient buffer and cls_hidden <= 1,024.  Combines with the plain cross entropy and with m2f_plan_focal (the focal factor scales
 * the emotion term only); refused while m2f_plan_distill, m2f_plan_rdrop, m2f_plan_crf or m2f_plan_supcon is on (the tail's fourth float
 * and the join point are taken), and each of them refuses while this is on.  A non-NULL param_grad is refused while the plan accumulates
 * gradients (m2f_plan_accumulate_grads) and by the split step (m2f_step_part), and they refuse it: that gradient would need the group's
 * den / an all-reduce.  A frozen head works with all of them. */
int m2f_plan_aux_head(m2f_plan* plan, const float* params, float* param_grad, int num_aux);

/* Linear-chain CRF criterion (the kernel-level entries m2f_crf_* below define it): while m2f_plan_crf(plan, params, param_grad) is on,
 * the criterion launch of m2f_loss / m2f_step / m2f_step_part / m2f_step_timed is the CRF loss over the plan's own dialogues (padded and
 * bucket-padded plans: rows b*L + i; packed and long-dialogue plans: the plan's cu_seqlens) with the same loss_terms / loss tail
 * (token_mean: num = logZ - score(y) per dialogue, den = labelled rows), and m2f_eval_step scores that loss (the train kernel's bits)
 * and counts the labels against the VITERBI path over the rows that are not padding instead of the per-row argmax.  label_smoothing
 * and class weights are not read.  params: device float [C*C + 2C] = [transitions | start | end], 16-byte aligned, the CALLER's (as
 * m2f_plan_stream_speakers takes its buffer): it is not in the flat parameter buffer, m2f_config or any optimizer table, and its VALUES
 * are read on the device at every step - a captured step replays while an optimizer updates them in place.  param_grad: device float
 * [C*C + 2C], overwritten by every step with the block's gradient (divided by den when the step normalises), the dialogues' shares
 * added in a fixed order; NULL: the block is frozen, a pure input.  params NULL: off.
 * Excludes m2f_plan_distill and m2f_plan_focal (each refuses the other by name).  A non-NULL param_grad is refused while the plan
 * accumulates gradients (m2f_plan_accumulate_grads) and by the split step (m2f_step_part), and they refuse it: that gradient would need
 * the group's den / an all-reduce.  A frozen block works with all of them.  A change of the pointers or the switch bumps the plan's
 * generation; a change of the values does not.  Train and eval plans with 2 .. 16 classes. */
int m2f_plan_crf(m2f_plan* plan, const float* params, float* param_grad);

/* The CRF's online form on a stream (m2f_crf_filter below): while m2f_plan_stream_crf(plan, params, phi) is on, m2f_stream_step (a
 * stream plan) / m2f_stream_prefill (a chunk plan) run the forward filter over the new utterances' logits behind the classifier and in
 * front of the launch that advances the counters, inside the same captured graph.  phi: the CALLER's device float [S, C], the slots'
 * filter state - log P(label of the slot's last utterance | its dialogue so far), the end term not applied; a slot whose count is 0
 * starts from `start`, whatever phi holds.  params as m2f_plan_crf (read on the device at every call).  A stream plan and its chunk
 * plan take the same two pointers.  Both NULL: off.  The logits are unchanged either way.  C floats per slot: no window limits it. */
int m2f_plan_stream_crf(m2f_plan* plan, const float* params, float* phi);

/* The 256x256-tile bf16 GEMM on the eight-phase schedule (csrc/gemm_p8.h; round 4), bf16 operands handed over directly - the kernel
 * the weight-gradient table launch (rc = 1) and the text encoder's launches (rc = 0) run, for kernel-level tests and measurements.
 *   rc = 0: C[M,N] = act(A[M,K] B[N,K]^T + bias) + res   (nn.Linear forward: src/feature_extractors/text/model.py:16-21's encoder
 *           layers); K % 64 == 0; act 0 none, 1 ReLU, 2 GELU
 *   rc = 1: C[M,N] = A[K,M]^T B[K,N]   (weight gradient dW = dY^T X of every nn.Linear in src/model.py: reduction over the token rows),
 *           relu_a / relu_b on the operands, bias_grad[M] = column sums of A (nullable); runs as a one-problem table launch whose table,
 *           tile records and per-workgroup ranges are written to `scratch` (device memory, >= 64 KiB + 4 bytes per tile) for n_wg
 *           workgroups (<= 0: 256); scratch_bytes < 0: `scratch` (of -scratch_bytes bytes) still holds the tables of an identical earlier call.
 * Returns 0, or < 0 when the shape / alignment is not this kernel's (no fallback). */
int m2f_gemm_p8(int rc, int M, int N, int K, const uint16_t* a, int lda, const uint16_t* b, int ldb, float* c, int ldc,
                const float* bias, const float* res, int ldres, int act, int relu_a, int relu_b, float* bias_grad,
                void* scratch, int64_t scratch_bytes, int n_wg, m2f_stream_t stream);
/* ---- dialogue attention: six launch entries, their options in two descriptors ----------------------------------------------------
 * One entry per launch kind - m2f_attention_fwd / _bwd (L <= 64), m2f_attention_varlen_fwd / _bwd (L <= 512), m2f_attention_stream
 * (one new utterance per slot) and m2f_attention_stream_chunk (up to T) - and every option of a forward launch is a FIELD of the
 * descriptor its last argument points to.  opts == NULL is the plain launch; a field at its "off" value runs the kernels of the launch
 * without it, bit for bit.  A new option is one more field (and one more template flag of the kernels), never one more entry.
 * Refused before any launch, with a message that names the entry: a gain that is negative, not finite or out of bf16's range;
 * negative head counts, n_same + n_other > H, a NULL speakers / spk_cache / spk_new with a non-zero count; paging arguments as below;
 * a misaligned weights buffer, and any weights buffer at the chunk entry.
 *
 * past / future - CONTEXT BAND (attn_mask of a band shape): >= 0, or negative = unlimited on that side.  Query i sees key j iff j is a
 *   valid key and j >= i - past and j <= i + future, i and j being utterance positions inside the dialogue (padded rows: the slot;
 *   packed rows: the row minus cu[b]).  (-1, 0) is causal attention, (k, 0) "the last k utterances and this one", (-1, -1) no band.  A
 *   hidden key has P = 0 exactly.  A query that sees NO key (a pad slot whose band holds pad keys only; a valid query always sees
 *   itself) gets a zero row of P, a zero output row and zero gradient terms, where torch's masked softmax gives NaN: such rows are pad
 *   rows of saved activations, and the weight gradients sum over every row.  The long-dialogue kernels (varlen) skip every pair of
 *   64-row blocks the band hides as a whole and leave its block of `probs` unwritten; the backward entries take the band as two plain
 *   arguments and must be given the band of the forward whose probabilities they read (the short backward does not read it: the saved
 *   P^T carries the band).  A ZERO-FILLED m2f_attn_opts is therefore a band of width zero, not "no option": start from
 *   M2F_ATTN_OPTS_NONE.
 * bias_gain - DISTANCE-DECAY BIAS (ALiBi): a VISIBLE key's score is fma(-slope, float(|i - j|), dot(q_i, k_j) * (1 / sqrt(hd))), all
 *   fp32 (in bf16 mode too: behind the contraction), i and j the positions the band compares; a hidden key stays -inf.  slope = gain *
 *   base(h, H), h the 0-based head: with n = 2^floor(log2 H), base = 2^(-8 (h + 1) / n) for h < n and 2^(-4 (2 (h - n) + 1) / n) for
 *   h >= n (H = 4: 1/4, 1/16, 1/64, 1/256; H = 3: 1/16, 1/256, 1/4).  gain >= 0 and finite, used as rounded to bf16 (what a plan
 *   applies); 0 = off.  The new utterance of a stream is at distance 0, cached utterance u at distance count - u.  The backward entries
 *   read the probabilities the biased forward saved and take no gain.
 * n_same / n_other - SPEAKER HEADS (m2f_plan_attention_speakers has the rule): heads 0 .. n_same - 1 see the keys of the query's own
 *   speaker only, the next n_other heads the keys of the other speakers only; (0, 0) = off.  speakers: device uint8, one id per token row
 *   (padded: [B*L]; packed: [T], row cu[b] + i).  Stream entries: spk_cache = device uint8 [S][C], the ids of the cached utterances by
 *   logical cache row (read only; the row the new utterance takes is never read), spk_new = device uint8 [S] (step) / [S][T] (chunk),
 *   the new utterances' ids.  An other-speaker head with no other speaker in sight gives a zero output row and a zero weights row.
 * table, table_cols, n_pages, page_rows - PAGED caches (layout: m2f_plan_create_stream_paged): table == NULL = dense caches, the three
 *   integers ignored; otherwise kcache / vcache are the POOLS [n_pages][H][page_rows][pad(hd)], m2f_attention_stream_pool_elems elements
 *   each, 16-byte aligned, and table is device int32 [S, table_cols], table_cols = ceil(C / page_rows).  Same results, bit for bit, as
 *   the dense launch on caches that hold the same rows.  Refused: page_rows outside {16, 32, 64}, misaligned pools, table_cols !=
 *   ceil(C / page_rows), n_pages < 1, C > 512, hd > 128.
 * weights - step entry only: the launch also stores each (slot, head)'s row of attention probabilities, fp32 [S, H, C], in LOGICAL
 *   order - column t is the t-th oldest live utterance of the slot, the last live column the utterance that has just arrived (a ring:
 *   utterance u sits in row u % C, undone here; paged: the page table never enters) - zeros behind the live count min(count + 1, C) and
 *   for inactive slots.  Same out, same cache rows, same bits.  NULL = off; the chunk entry has no such kernel and refuses a buffer. */
typedef struct m2f_attn_opts {          /* forward of the short and long-dialogue kernels */
    int past, future;                   /* context band, negative = unlimited on that side */
    float bias_gain;                    /* distance-decay gain, 0 = off (applied as rounded to bf16) */
    int n_same, n_other;                /* speaker heads, (0, 0) = off */
    const uint8_t* speakers;            /* one id per token row; needed iff n_same | n_other */
} m2f_attn_opts;
#define M2F_ATTN_OPTS_NONE {-1, -1, 0.f, 0, 0, NULL}        /* "no option": what opts == NULL means */
typedef struct m2f_attn_stream_opts {   /* stream step and chunk; zero-filled = no option */
    const int32_t* table; int table_cols, n_pages, page_rows;   /* table NULL = dense caches, else kcache / vcache are the pools */
    float* weights;                     /* step only: [S, H, C] rows of probabilities, NULL = off */
    float bias_gain;
    int n_same, n_other; const uint8_t* spk_cache; const uint8_t* spk_new;
} m2f_attn_stream_opts;
/* sizeof and the field offsets, in declaration order, of m2f_attn_opts - which = 0 - or m2f_attn_stream_opts - which = 1 - as this library
 * was compiled: up to max ints into out; returns how many there are, < 0 for another `which`.  Host only (bindings check their mirror). */
int m2f_attention_opts_layout(int which, int* out, int max);
/* softmax(q k^T / sqrt(hd) + key_padding_mask) v per (dialogue, head) (nn.MultiheadAttention inside
 * src/model.py:8,14,61,73); probs receives P^T per head, padded to Lp = 16*ceil(L/16). */
int m2f_attention_fwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                      const float* v, int ldv, const uint8_t* key_pad, float* out, int ldo, float* probs,
                      uint32_t drop_site, float drop_p, const uint32_t* rng_state, m2f_stream_t stream, const m2f_attn_opts* opts);
int m2f_attention_bwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                      const float* v, int ldv, const uint8_t* key_pad, const float* out, int ldo,
                      const float* probs, const float* dout, int lddo, float* dq, int lddq, float* dk,
                      int lddk, float* dv, int lddv, uint32_t drop_site, float drop_p,
                      const uint32_t* rng_state, m2f_stream_t stream, int past, int future);
int64_t m2f_attention_probs_elems(int B, int H, int L);
/* The attention map of ONE site out of the probs that m2f_attention_fwd / m2f_attention_varlen_fwd wrote for the same
 * B, L, H (csrc/attention_weights.hip; m2f_plan_attention_weights above has the rule): out = fp32 [B, H, L, L] (per_head) or [B, L, L]
 * (heads summed in order, times (float)1 / H).  key_pad (padded rows, [B, L]) or cu (packed rows, int32 [B + 1]) or neither (every key
 * valid); past / future: the band the forward ran under (negative = unlimited).  Elements outside the dialogue, at padded keys or
 * hidden by the band are written as 0 and never read from probs.  1 <= L <= 512. */
int m2f_attention_weights(int B, int L, int H, const float* probs, const uint8_t* key_pad, const int32_t* cu, int past, int future,
                          int per_head, float* out, m2f_stream_t stream);
/* Streaming attention, one launch (csrc/attention_stream.hip): slot s of S takes ONE new utterance - rows s of q / k / v [S, H*hd] fp32,
 * column slices with their leading dimensions - against the rows the slot has cached.  count[s] (device int32) = utterances cached so far,
 * active[s] (device uint8).  An active slot: the new K / V rows are stored at row count % C (ring != 0) or row count (ring == 0;
 * count < C required) of kcache / vcache, and out[s] = softmax(q K^T / sqrt(hd)) V over the min(count + 1, C) live rows, the new one
 * included (count == 0: the new V row itself).  An inactive slot: out[s] = 0, caches untouched.  count is NOT advanced.  Caches:
 * [S][H][C][pad4(hd)] float (bf16 == 0) or [S][H][C][pad8(hd)] bf16 (bf16 != 0: K, V rounded once on the way in, q where it enters
 * the product, softmax and sums fp32), 16-byte aligned, m2f_attention_stream_cache_elems elements each.  hd <= 128, C <= 512. */
int64_t m2f_attention_stream_cache_elems(int S, int H, int hd, int C, int bf16);
int64_t m2f_attention_stream_pool_elems(int n_pages, int H, int hd, int page_rows, int bf16);
int m2f_attention_stream(int S, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                         void* kcache, void* vcache, int C, int ring, const int32_t* count, const uint8_t* active, float* out, int ldo,
                         int bf16, m2f_stream_t stream, const m2f_attn_stream_opts* opts);
/* The chunk form, one launch (csrc/attention_stream_chunk.hip): slot s takes n_new[s] (device int32, 0 .. T, T <= 64) new utterances -
 * rows s*T + t of q / k / v / out [S*T, H*hd] - and gets, row by row, what n_new[s] launches of m2f_attention_stream give: row t
 * attends to the chunk's rows <= t and to the cached utterances (ring != 0: to the last C - 1 utterances before it only), the chunk's
 * own keys and values taken from the rows given (bf16 != 0: rounded once), never through the cache.  The new K / V rows are stored
 * at rows (count + t) % C (ring) or count + t (ring == 0; count + n_new <= C required, else the slot is left untouched) after the
 * launch's last cache read; of n_new > C rows on a ring the last C.  Output rows t >= n_new[s] are zeros and their input rows are
 * never read; n_new[s] == 0 leaves the slot's caches untouched.  count is NOT advanced. */
int m2f_attention_stream_chunk(int S, int T, int H, int hd, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                               void* kcache, void* vcache, int C, int ring, const int32_t* count, const int32_t* n_new, float* out, int ldo,
                               int bf16, m2f_stream_t stream, const m2f_attn_stream_opts* opts);
/* The launch that closes a step / a prefill call of a stream with speaker heads: the new ids into the rows the new utterances took
 * (what the attention launch did with K / V), then count += active (or the clamped n_new).  m2f_attention_speaker_class: 0 untouched,
 * 1 same-speaker, 2 other-speaker. */
int m2f_stream_advance_speakers(int S, int C, int ring, int32_t* count, const uint8_t* active, uint8_t* spk_cache, const uint8_t* spk_new,
                                m2f_stream_t stream);
int m2f_stream_advance_speakers_n(int S, int T, int C, int ring, int32_t* count, const int32_t* n_new, uint8_t* spk_cache, const uint8_t* spk_new,
                                  m2f_stream_t stream);
int m2f_attention_speaker_class(int h, int n_same, int n_other);
/* Snapshot / restore of ONE site's stream caches (csrc/stream_cache.hip): the live rows of listed slots <-> a packed buffer.  Entry e
 * of n_entries holds the rows = min(lengths[e], C) live PHYSICAL cache rows 0 .. rows - 1 of slot slots[e] (a ring keeps its phase) as
 * [K, V][H][rows][pad(hd)] - the dense cache with C replaced by rows, pad columns as they are - and starts at element
 * row_offsets[e] * 2 * H * pad(hd) of `packed` (16-byte aligned, packed_elems elements of the caches' type).  slots, lengths (device
 * int32) and row_offsets (device int64) have n_entries entries.  gather: caches -> packed, the caches are only read.  scatter:
 * packed -> caches and count[slot] = lengths[e] (an entry of length 0 resets its slot); rows >= min(lengths[e], C) of a listed slot,
 * every other slot and - paged - every other page are not written; the caller lists a slot once and keeps lengths <= C on a plain
 * cache.  An entry out of range (slot outside 0 .. S - 1, negative length or offset, rows past packed_elems) is skipped whole.
 * table / table_cols / n_pages / page_rows: the paging fields of m2f_attn_stream_opts as plain arguments (table == NULL: dense caches);
 * the table is read only at the entries of pages that hold a row of the entry, and the packed bytes do not depend on the form.
 * Argument checks as m2f_attention_stream. */
int m2f_attention_stream_cache_gather(int S, int H, int hd, const void* kcache, const void* vcache, const int32_t* table, int table_cols,
                                      int n_pages, int page_rows, int C, int bf16, int n_entries, const int32_t* slots,
                                      const int32_t* lengths, const int64_t* row_offsets, void* packed, int64_t packed_elems,
                                      m2f_stream_t stream);
int m2f_attention_stream_cache_scatter(int S, int H, int hd, void* kcache, void* vcache, const int32_t* table, int table_cols,
                                       int n_pages, int page_rows, int C, int bf16, int n_entries, const int32_t* slots,
                                       const int32_t* lengths, const int64_t* row_offsets, const void* packed, int64_t packed_elems,
                                       int32_t* count, m2f_stream_t stream);
/* The same attention for dialogues of up to 512 utterances (the kernels packed plans with L > 64 run): one workgroup per 64-row
 * block of a (dialogue, head), keys streamed in 64-row blocks.  Rows are given in one of two forms:
 *   packed: cu (int32 [B+1], device) - dialogue b owns rows cu[b] .. cu[b+1]-1 (at most L of them), T rows in all; rows cu[B] ..
 *           T-1 of out (dq / dk / dv) are written as zeros; key_pad = NULL;
 *   padded: key_pad (uint8 [B*L], 1 = padded key, masked with -inf before the softmax) - dialogue b owns rows b*L .. b*L+L-1; cu = NULL.
 * probs receives P^T (pre-dropout) in the layout of m2f_attention_fwd, [B*H, Lp, Lp] (m2f_attention_probs_elems); the backward
 * reads it back (no recompute) and replays dropout from the same keep index.  1 <= L <= 512, hd <= 256, B * H * L * L < 2^32.
 * Deterministic: every result element is written by one workgroup, no atomics. */
int m2f_attention_varlen_fwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                             const float* v, int ldv, const int32_t* cu, int T, const uint8_t* key_pad, float* out, int ldo,
                             float* probs, uint32_t drop_site, float drop_p, const uint32_t* rng_state, m2f_stream_t stream,
                             const m2f_attn_opts* opts);
int m2f_attention_varlen_bwd(int B, int L, int H, int hd, const float* q, int ldq, const float* k, int ldk,
                             const float* v, int ldv, const int32_t* cu, int T, const uint8_t* key_pad, const float* out, int ldo,
                             const float* probs, const float* dout, int lddo, float* dq, int lddq, float* dk, int lddk,
                             float* dv, int lddv, uint32_t drop_site, float drop_p, const uint32_t* rng_state,
                             m2f_stream_t stream, int past, int future);
/* out = (res ? res : 0) + LayerNorm(x) (nn.LayerNorm, eps), stats[T,2] = (mean, rstd). */
int m2f_layernorm_fwd(int T, int d, const float* x, const float* gamma, const float* beta, const float* res,
                      float* out, float* stats, float eps, m2f_stream_t stream);
/* dx = LayerNorm backward (+extra); dgamma/dbeta via per-block partials (partial: [ceil(T/4), 2, d]). */
int m2f_layernorm_bwd(int T, int d, const float* x, const float* gamma, const float* stats, const float* dy,
                      const float* extra, float* dx, float* partial, float* dgamma, float* dbeta,
                      m2f_stream_t stream);
/* The row-wise kernels with a dropout site, as the train plans launch them (kernel-level tests; no kernel of their own).  Rows have
 * d elements and stride ld (0 = d); the keep index of element (row, col) is row * d + col, whatever ld.  drop_p > 0 and rng_state
 * (4 device uint32) are needed when a site is non-zero.
 * m2f_layernorm_fwd_drop: out = dropout_site((res ? res : 0) + LayerNorm(x)) - the pre-projection dropout on the last encoder stack's
 * final norm. */
int m2f_layernorm_fwd_drop(int T, int d, int ld, const float* x, const float* gamma, const float* beta, const float* res, float* out,
                           float* stats, float eps, uint32_t drop_site, float drop_p, const uint32_t* rng_state, m2f_stream_t stream);
/* m2f_layernorm_bwd_masked: m2f_layernorm_bwd with the second output dx_masked = LNbwd(dy) * keep(drop_site2) / (1 - p) (nullable;
 * without `extra`: what flows on through dropout1 / dropout2), dx = LNbwd(dy) (+ extra) as ever. */
int m2f_layernorm_bwd_masked(int T, int d, int ld, const float* x, const float* gamma, const float* stats, const float* dy,
                             const float* extra, float* dx, float* dx_masked, float* partial, float* dgamma, float* dbeta,
                             uint32_t drop_site2, float drop_p, const uint32_t* rng_state, m2f_stream_t stream);
/* m2f_dropout_rows: in place x[t, c] *= keep(site, t * d + c) / (1 - p) for c < d; x2 (nullable): a second buffer of the same shape
 * with its own site in the same launch (the two modalities' post-projection gradients). */
int m2f_dropout_rows(float* x, float* x2, int T, int d, int ld, uint32_t site, uint32_t site2, float drop_p, const uint32_t* rng_state,
                     m2f_stream_t stream);
/* CrossEntropyLoss(ignore_index=-1, label_smoothing[, weight]) + gradient; loss_out[0..2] = loss, den, num. */
int m2f_cross_entropy(int T, int C, const float* logits, const int64_t* labels, const float* class_w,
                      float label_smoothing, int normalise, float* loss_terms, float* dlogits, float* loss_out,
                      m2f_stream_t stream);
/* The distillation criterion of m2f_plan_distill on its own: m2f_cross_entropy with teacher logits [T, C] and hyper_dev (device
 * float [2]: alpha in [0, 1], tau > 0). */
int m2f_cross_entropy_distill(int T, int C, const float* logits, const float* teacher, const int64_t* labels, const float* class_w,
                              float label_smoothing, const float* hyper_dev, int normalise, float* loss_terms, float* dlogits,
                              float* loss_out, m2f_stream_t stream);
/* The focal criterion of m2f_plan_focal on its own: m2f_cross_entropy with gamma_dev (device float [1], gamma in [0, 8]).  teacher
 * [T, C] with hyper_dev (device float [2]: alpha, tau) adds the distillation blend of m2f_cross_entropy_distill; teacher NULL: no
 * distillation, hyper_dev is not read. */
int m2f_cross_entropy_focal(int T, int C, const float* logits, const float* teacher, const int64_t* labels, const float* class_w,
                            float label_smoothing, const float* hyper_dev, const float* gamma_dev, int normalise, float* loss_terms,
                            float* dlogits, float* loss_out, m2f_stream_t stream);
/* The R-Drop criterion of m2f_plan_rdrop on its own: m2f_cross_entropy with partner (device int32 [T]: the twin ROW of every row of
 * logits, or -1) and alpha_dev (device float [1], alpha >= 0).  loss_terms: scratch of 3 * T floats here ([T, 2] numerator / denominator,
 * then [T] w_y * s_r); loss_out[3] = sum w_y * s_r (the KL share of the numerator is alpha times it). */
int m2f_cross_entropy_rdrop(int T, int C, const float* logits, const int32_t* partner, const int64_t* labels, const float* class_w,
                            float label_smoothing, const float* alpha_dev, int normalise, float* loss_terms, float* dlogits,
                            float* loss_out, m2f_stream_t stream);

/* The supervised contrastive kernels on their own (csrc/supcon.hip).  features: [N, D] fp32 with row stride ld >= D; labels int64 [N] (a
 * label outside [0, C) = not in V); class_w [C] or NULL; hyper_dev: device float [2] = (lambda >= 0, tau > 0).  scratch: device buffer of
 * m2f_supcon_scratch_floats(N, D) floats, 16-byte aligned.  Outputs: row_terms [N, 4] = (lse_i, n_i, l_i, w_{y_i} l_i), 16-byte aligned -
 * zeros outside V, l = 0 for a row of V without a positive -, and dfeatures [N, D] (row stride ldd >= D) =
 *   dz_i = (1 / tau) sum_{a in A(i)} [c_i (p_ia - m_ia / n_i) + c_a (p_ai - m_ia / n_a)] z_a,   dh_i = (dz_i - (dz_i . z_i) z_i) / ||h_i||
 * with c_i = lambda * w_{y_i} * [n_i > 0], p_ia = exp(s_ia - lse_i), m_ia = [y_i = y_a]: the gradient of lambda * sum_i w_{y_i} l_i,
 * zeros outside V.  Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, every sum in one fixed order: the same bits at every call. */
int64_t m2f_supcon_scratch_floats(int N, int D);
int m2f_supcon(int N, int D, int C, const float* features, int ld, const int64_t* labels, const float* class_w, const float* hyper_dev,
               float* scratch, float* row_terms, float* dfeatures, int ldd, m2f_stream_t stream);

/* The auxiliary label head's kernels on their own (csrc/aux_head.hip).  features: [N, D] fp32 with row stride ld >= D, ld a multiple of 4
 * and the rows 16-byte aligned, D <= 1,024; params [A * D + A] = [W | b], 16-byte aligned, 2 <= A <= 16; labels / aux_labels int64 [N]
 * (a label outside [0, C) / [0, A) = ignored row); class_w [C] or NULL; hyper_dev: device float [2] = (lambda >= 0, 0 <= eps_a < 1).
 * scratch: device buffer of m2f_aux_head_scratch_floats(N, D, A) floats, 16-byte aligned.  Outputs: aux_logits [N, A] = W h + b (every
 * row), row_terms [N] = w_y a_i (0 on an ignored row), dfeatures [N, D] (row stride ldd as ld) = lambda * sum_c g[i, c] W[c, :] - the
 * gradient of lambda * sum_i w_y a_i, NO gate, exact zeros on an ignored row - and, dparams non-NULL, dparams [A * D + A] = lambda *
 * [g^T h | sum_i g_i] (a row with g = 0 is SELECTED out: its h may hold anything).  No atomics, every sum in one fixed order. */
int64_t m2f_aux_head_scratch_floats(int N, int D, int A);
int m2f_aux_head(int N, int D, int A, int C, const float* features, int ld, const float* params, const int64_t* labels,
                 const int64_t* aux_labels, const float* class_w, const float* hyper_dev, float* scratch, float* aux_logits,
                 float* row_terms, float* dfeatures, int ldd, float* dparams, m2f_stream_t stream);
/* The head under autograd (multimodal-emotion-recognition_amd/aux_head.py): logits [N, A] = W h + b, and, from an upstream gradient
 * g [N, A], dfeatures [N, D] = g W (NULL: skipped) and dparams = [g^T h | sum_i g_i] (NULL: skipped) - the same kernels.  scratch as above. */
int m2f_aux_head_forward(int N, int D, int A, const float* features, int ld, const float* params, float* scratch, float* logits,
                         m2f_stream_t stream);          /* scratch: unused by the forward, may be NULL */
int m2f_aux_head_backward(int N, int D, int A, const float* features, int ld, const float* params, const float* g, float* scratch,
                          float* dfeatures, int ldd, float* dparams, m2f_stream_t stream);

/* The join launch of the step on caller-owned buffers: dh[i, :] = (add: dh[i, :] +) gate * scale * lambda * sum_c g[i, c] W[c, :] with
 * gate = (h[i, :] > 0 ? gate_scale : 0), or 1 with h NULL; scale = scale_dev[0], lambda = hyper_dev[0] (device floats; NULL: 1).  dh [N, D]
 * with row stride ldd, h with ld (16-byte aligned rows, strides multiples of 4), g [N, A] with row stride ldg.  shadow non-NULL: uint16
 * [N * ldd], element e receives the bf16 rounding (nearest even) of dh[e] as written - what the step does to the plan's activation shadow
 * in bf16 mode; columns behind D are not touched in either buffer. */
int m2f_aux_head_join(int N, int D, int A, float* dh, int ldd, const float* h, int ld, const float* g, int ldg, const float* params,
                      const float* scale_dev, const float* hyper_dev, float gate_scale, int add, uint16_t* shadow, m2f_stream_t stream);

/* ---- linear-chain CRF over a dialogue's labels (multimodal-emotion-recognition_amd/crf.py, csrc/crf.hip) --------------------------
 * params: float [C*C + 2C] = [transitions row-major C x C | start C | end C], 2 <= C <= 16.  The block is NOT part of the flat parameter
 * buffer or of m2f_config: the caller owns it.  Dialogue b owns token rows cu_seqlens[b] .. cu_seqlens[b+1]-1 (int32 [B+1], device) or,
 * cu_seqlens NULL, rows b*L .. b*L+L-1 (B * L <= T).  Rows outside every dialogue get zeros / -1.
 *
 * m2f_crf_nll: the chain of a dialogue is its rows with a label in [0, C), in row order (a -1 in the middle links its neighbours; the
 * logits of an unlabelled row are never read).  For chain rows t_1 < ... < t_n with emissions e = logits and labels y:
 *   score(y) = start[y_1] + sum_k e[t_k, y_k] + sum_{k>=2} transitions[y_{k-1}, y_k] + end[y_n],  logZ = log sum_paths exp(score)
 *   loss_terms [T, 2]: num = logZ - score(y) on the dialogue's first chain row, den = 1 on every chain row;
 *   loss_out [4] = loss (sum num / sum den: token_mean), den, num, -   as m2f_cross_entropy
 *   dlogits [T, C] = P(y_k = c) - [c == y_k] on chain rows, 0 elsewhere; divided by den when normalise != 0; NULL (with param_grad
 *   NULL): the loss alone - the forward sweep, no gradient (what m2f_eval_step runs)
 *   param_grad [C*C + 2C] (NULL: the parameters are frozen, nothing is computed for them): d transitions, d start, d end in the layout of
 *   params, the dialogues' shares added in dialogue order without atomics (same bits every run); divided by den when normalise != 0 (a batch without any labelled row: zeros, where loss and dlogits are 0 / 0 as the plain criterion's).
 * alpha is carried normalised in log space and the marginals are formed from relative values: fp32 results stay within ~1e-6 of
 * float64 at 512 rows, and transitions of -1e4 or logit margins of +-120 stay finite.  A dialogue without a chain row contributes
 * nothing.  scratch: m2f_crf_scratch_floats(T, B, C) floats.  Three launches (two without param_grad), nothing waited for.
 *
 * m2f_crf_viterbi: the chain is the rows whose mask (uint8 [T]) is 0.  pred [T] = the best path's class, -1 off the chain; score [B] =
 * the path's score (0 without a chain row).  The lowest class wins every tie.  scratch: 20 * T bytes (m2f_crf_scratch_floats covers it).
 *
 * m2f_crf_filter: the online form, for stream slots.  phi [S, C] in and out: log P(label of the slot's last utterance | the dialogue so
 * far), the end term not applied.  Slot s takes rows s*rows .. s*rows + n_new[s] - 1 of logits [S*rows, C] in order (n_new NULL, rows
 * == 1: one row); active (uint8 [S], NULL: all) = 0 leaves the slot untouched.  count [S] int32 = utterances the slot held before the
 * call (0: the first row starts from `start`); it is read, never written.  One row per call n times gives the bits of n rows at once. */
int64_t m2f_crf_scratch_floats(int T, int B, int C);
int m2f_crf_nll(int T, int C, int B, int L, const int32_t* cu_seqlens, const float* logits, const int64_t* labels, const float* params,
                int normalise, float* scratch, float* loss_terms, float* dlogits, float* param_grad, float* loss_out,
                m2f_stream_t stream);
int m2f_crf_viterbi(int T, int C, int B, int L, const int32_t* cu_seqlens, const float* logits, const uint8_t* mask, const float* params,
                    void* scratch, int32_t* pred, float* score, m2f_stream_t stream);
int m2f_crf_filter(int S, int C, int rows, const float* logits, const float* params, const int32_t* count, const uint8_t* active,
                   const int32_t* n_new, float* phi, m2f_stream_t stream);

/* ---- wav2vec2 audio encoder (multimodal-emotion-recognition_amd/wav2vec2.py) ------------------------------------------------------
 * The reference makes its audio embeddings in a separate stage (src/feature_extractors/audio_wav2vec2/embeddings.py:52-91:
 * torchaudio WAV2VEC2_BASE on batches of zero-padded 16 kHz waveforms, then the mean of each utterance's valid frames).  These
 * entries are the kernels of that model the GEMM / attention / LayerNorm entries do not cover.  Activations are channels-last; all
 * are deterministic (no atomics, fixed reduction orders).
 *
 * Conv layer 0 (Conv1d(1, C, k0, stride s0, bias=False)) + GroupNorm(C, C) + exact GELU (torchaudio ConvLayerBlock 0; the
 * reference's embeddings.py:77 call model(audio, lengths)): wave [B, N] fp32, the padded batch; w0 [C, k0]; the statistics of channel
 * c of utterance b cover frames 0 .. T0-1 of the PADDED waveform (T0 = (N - k0) / s0 + 1), so a short utterance's output depends on
 * the longest one in its batch, as in the reference.  Output row b * P0 + t (P0 >= T0; rows T0 .. P0-1 are written as zeros) of
 * exactly one of out32 (fp32) / out16 (bf16 bits), C columns.  partial / stats: device scratch of
 * m2f_w2v_conv0_scratch_floats(B, C, T0) floats, partial first, then stats (B * C * 2).  k0 <= 16, s0 <= 8. */
int m2f_w2v_conv0(int B, int N, const float* wave, const float* w0, int k0, int s0, int C, int T0, int P0, const float* gamma,
                  const float* beta, float eps, float* scratch, float* out32, uint16_t* out16, m2f_stream_t stream);
int64_t m2f_w2v_conv0_scratch_floats(int B, int C, int T0);
/* Feature-projection LayerNorm (torchaudio FeatureProjection.layer_norm) with the row compaction of the conv stack folded into its
 * read: row b * P + t of x [B * P, C] -> row b * S + t of out32 [B * S, C] (and of out16, bf16 bits, when non-NULL).  C <= 1024. */
int m2f_w2v_feat_layernorm(int B, int S, int P, int C, const float* x, const float* gamma, const float* beta, float eps, float* out32,
                           uint16_t* out16, m2f_stream_t stream);
/* Positional convolution + residual (torchaudio ConvolutionalPositionalEmbedding, Conv1d(d, d, K, padding K/2, groups), weight norm
 * folded into w; the extra last frame of an even K dropped; then x + GELU(conv(x))):
 *   out[b*S + t, g*CG + o] = GELU(bias + sum_{k<K, c<CG} x[t + k - K/2, g*CG + c] w[g][k][o][c]) + x[t, g*CG + o]
 * with rows of x at or past lengths[b] (int32, device) read as zero, the residual included.  x, out [B*S, d] fp32; CG = d / groups
 * in {16, 32, 48, 64}; K <= 256.  bf16 = 0: w fp32, exact-fp32 MFMA; bf16 = 1: w bf16 bits, x rounded to bf16, fp32 accumulation. */
int m2f_w2v_pos_conv(int B, int S, int d, int groups, int K, const float* x, const int32_t* lengths, const void* w, const float* bias,
                     float* out, int bf16, m2f_stream_t stream);
/* out[b, c] = mean of x[b*S + t, c] over t < lengths[b] (embeddings.py:80-85; fixed summation order, lengths[b] <= 0 gives zeros). */
int m2f_w2v_masked_mean(int B, int S, int d, const float* x, const int32_t* lengths, float* out, m2f_stream_t stream);

/* ---- audio_mel encoder (multimodal-emotion-recognition_amd/mel_resnet.py) ---------------------------------------------------------
 * The reference's third per-utterance feature extractor (src/feature_extractors/audio_mel): a log-mel spectrogram of each utterance,
 * min-max normalised (and, as its PNG cache returns it, quantised to 8-bit levels), as a [3, 1001, 128] image into torchvision's
 * resnet18, then ReLU -> Linear(1000, 300) -> L2 normalise.  Activations are NHWC; all entries are deterministic and per utterance.
 *
 * Front end: wave [B, N] fp32 (padded batch), lengths [B] int32 on the device (<= N, <= 160,000 samples); basis [400][402] = Hann
 * window x (cos | sin) of the 201 DFT bins; fbT [201][128] the mel filters (L1-normalised rows) transposed.  img [B, 1001, 128] fp32:
 * frames 0 .. len / 160 normalised to [0, 1] (floor(v * 255) / 255 when png_levels), zero rows behind them; a silent clip or a
 * flat spectrogram gives all zeros.  scratch: m2f_mel_frontend_scratch_floats(B) floats. */
int m2f_mel_frontend(int B, int N, const float* wave, const int32_t* lengths, const float* basis, const float* fbT, int png_levels,
                     float* scratch, float* img, m2f_stream_t stream);
int64_t m2f_mel_frontend_scratch_floats(int B);
/* Stem: 7x7/2 conv of img (one channel: the three identical input channels folded) + BatchNorm folded into w [49][64] (tap-major) and
 * bias [64] + ReLU + 3x3/2 max pool -> [B, 251, 32, 64] NHWC, exactly one of out32 (fp32) / out16 (bf16 bits).  fp32 arithmetic. */
int m2f_mel_stem(int B, const float* img, const float* w, const float* bias, float* out32, uint16_t* out16, m2f_stream_t stream);
/* Convolution (implicit GEMM, no im2col): x [B, H, W, Cin], w [Cout][ks][ks][Cin] (BatchNorm folded), pad ks / 2, out / res
 * [B, Ho, Wo, Cout]: out = act(conv(x) + bias (+ res)), act = ReLU when relu.  bf16 = 0: x, w, res, out fp32 (fp32 MFMA); bf16 = 1:
 * x, w, res bf16 bits, fp32 accumulation, out bf16 bits (fp32 when out_fp32).  Cin % 32 == 0, Cout % 64 == 0, ks 1 or 3, stride 1 or 2. */
int m2f_mel_conv(int B, int H, int W, int Cin, int Cout, int ks, int stride, const void* x, const void* w, const float* bias,
                 const void* res, void* out, int bf16, int out_fp32, int relu, m2f_stream_t stream);
/* Head: x [B, HW, C] (bf16 bits when bf16_in) -> mean over HW -> ReLU(. W1^T + b1) -> . W2^T + b2 -> / max(||.||, 1e-12): out [B, N2].
 * w1t [C][N1], w2t [N1][N2] (transposed Linear weights); fp32, fixed summation orders. */
int m2f_mel_head(int B, int HW, int C, const void* x, int bf16_in, const float* w1t, const float* b1, int N1, const float* w2t,
                 const float* b2, int N2, float* out, m2f_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* M2FNET_HIP_H */
