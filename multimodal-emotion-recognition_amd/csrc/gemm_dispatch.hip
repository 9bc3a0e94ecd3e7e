// GEMM dispatch (host only, no kernels): which kernel form a launch takes.  The one owner of that policy - the knobs, the eligibility
// predicates and the decision ladder (m2f_gemm_choose / m2f_gemm_choose_fp8) - shared by the launchers (m2f_launch_gemm,
// m2f_launch_gemm_fp8: validate, choose, execute the choice), by the plan (m2f_gemm_stages_bf16: which fp32 buffers no kernel reads)
// and by the tests (m2f_gemm_form: the chooser's answer for a synthetic batch, no GPU needed).  The kernels and their launch code live
// in gemm.hip (register-staged), gemm_ring_*.hip, gemm_p8.hip and skinny.hip.
#include "common.h"
#include "ops.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

long long m2f_g_ring_launches = 0;
int m2f_g_last_form = M2F_FORM_NONE;

extern "C" long long m2f_gemm_ring_launches(void) { return m2f_g_ring_launches; }
extern "C" int m2f_gemm_last_form(void) { return m2f_g_last_form; }

// ---- knobs ---------------------------------------------------------------------------------------------------------------------
const GemmKnobs& m2f_gemm_knobs() {
    static const GemmKnobs k = [] {
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        GemmKnobs v;
        // Forward-form launches run the ring form (gemm_ring.h, m2f_gemm16_ring_kernel): 128x128 tiles from ~one tile per CU
        // on, 128x64 tiles below that while those still cover most of the chip, 64x64 tiles for the rest down to 80 tiles;
        // what remains (a few tiles, e.g. the classifier) keeps the register-staged 64x64 build.  Measured on MI355X,
        // fwd+bwd of the C3 step (B = 64): 3.21 ms without the ring form; 3.06 with the 128x128 form from 200 tiles (3.07 /
        // 3.07 / 3.16 at 100 / 150 / 260); 2.91 with the 128x64 form from 150 tiles on top (2.95 / 2.91 at 200 / 100); 2.89
        // with the 64x64 form from 80 tiles (no change down to 1).  C2 (B = 32): 1.957 -> 1.914 -> 1.853 (the 128x64 form
        // from 100 tiles: 2.014 - launches of ~100 tiles leave too many CUs idle).  M2F_RING=0 switches the form off,
        // M2F_RING_MIN / M2F_RING64_MIN / M2F_RING32_MIN move the thresholds.
        v.ring = env("M2F_RING", 1);
        v.ring_min = env("M2F_RING_MIN", 200);               // tiles of 128x128
        v.ring64_min = env("M2F_RING64_MIN", 150);           // tiles of 128x64
        v.ring32_min = env("M2F_RING32_MIN", 80);            // tiles of 64x64
        // Text-encoder-sized launches (M = utterances x tokens = 32,768): 256x128 ring tiles, whose k-loop runs at the MFMA rate
        // (1,050 cycles per 256x128x64 k-tile against 1,024) and whose fixed cost per tile is amortised by the persistent walk.
        // RoBERTa-large geometry 50.2 -> 43.4 ms per forward, base 17.4 -> 14.5 (threshold 512 tiles; 15.0 at 1,024; no
        // launch of the M2FNet step is that large).
        v.ring256_min = env("M2F_RING256_MIN", 512);         // tiles of 256x128
        // launches of 257..511 tiles of 128x128 take two rounds on 256 CUs with the second one mostly empty (the merged audio +
        // text QKV in-projections at C3: 336 tiles); as 256x128 tiles they are one round (168 tiles).  M2F_RING256_2R=0 switches it off
        v.ring256_2r = env("M2F_RING256_2R", 1);
        // Round 4: from one chip-filling round of 256 x 256 tiles on, the eight-phase form (gemm_p8.h: all eight waves load and multiply,
        // continuous prefetch stream across tiles): 32,768 x 1,024 x 1,024 752 TFLOP/s against ~460 for the 256x128 ring form.
        // M2F_P8=0 switches it off, M2F_P8_MIN moves the threshold (tiles of 256x256); bf16 and fp8 launches alike.
        v.p8 = env("M2F_P8", 1);
        v.p8_min = env("M2F_P8_MIN", 256);
        // fp8: the ring form (gemm_ring_256x128_fp8.hip) from one chip-filling round of 256x128 tiles on; M2F_RING_FP8=0 keeps the
        // register-staged build
        v.ring_fp8 = env("M2F_RING_FP8", 1);
        // the classifier head's [T, n_classes] problems: FMA kernels over the whole chip instead of one column of MFMA tiles (skinny.hip)
        v.skinny = env("M2F_SKINNY", 1);
        return v;
    }();
    return k;
}

// ---- eligibility ---------------------------------------------------------------------------------------------------------------
namespace {

// B's bf16 shadow as the launch reads it: the transposed one (qt / ldqt) when an NN launch runs as the k-contiguous form
const uint16_t* bq_of(const GemmProblem& p, int s, bool b_t) { return b_t ? p.b.qt[s] : p.b.q[s]; }
int ldbq_of(const GemmProblem& p, int s, bool b_t) { return b_t ? p.b.ldqt[s] : p.b.ldq[s]; }

// can every operand of every problem be staged from its bf16 shadow with 16-byte loads?
bool src16_ok(const GemmBatch& gb, bool a_rc, bool b_rc, bool b_t) {
    auto seg_ok = [](const uint16_t* q, int ldq, int k, bool rc, int rows) {
        if (k == 0) return true;
        if (!q || (reinterpret_cast<uintptr_t>(q) & 15) || (ldq & 7)) return false;
        const int extent = rc ? rows : k;                    // the contiguous dimension
        if ((extent & 7) && ldq != ((extent + 7) & ~7)) return false;   // pads must be the buffer's own zero pads
        return ldq >= extent;
    };
    for (int i = 0; i < gb.count; ++i) {
        const GemmProblem& p = gb.pr[i];
        for (int s = 0; s < 2; ++s)
            if (!seg_ok(p.a.q[s], p.a.ldq[s], p.a.k[s], a_rc, p.M) || !seg_ok(bq_of(p, s, b_t), ldbq_of(p, s, b_t), p.b.k[s], b_rc, p.N)) return false;
    }
    return true;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// may the fp32-source kernels move this operand in 16-byte chunks?
bool vec_ok(const GemmOperand& o, bool rc, int rows) {
    for (int s = 0; s < 2; ++s) {
        if (o.k[s] == 0) continue;
        if (!aligned16(o.p[s]) || (o.ld[s] & 3)) return false;
        if (!rc && (o.k[s] & 3)) return false;
    }
    if (rc && (rows & 3)) return false;
    return true;
}

// 32-bit byte offsets into every operand of the LDS-DMA forms
bool operands_below_2gib(const GemmProblem& p, bool b_t) {
    for (int sgm = 0; sgm < 2; ++sgm)
        if ((size_t)p.M * p.a.ldq[sgm] * 2 >= 0x80000000ull || (size_t)p.N * ldbq_of(p, sgm, b_t) * 2 >= 0x80000000ull) return false;
    return true;
}

int count_tiles(const GemmBatch& gb, int bm, int bn) {
    int t = 0;
    for (int i = 0; i < gb.count; ++i) t += m2f_cdiv(gb.pr[i].M, bm) * m2f_cdiv(gb.pr[i].N, bn);
    return t;
}

}  // namespace

// can this forward-form launch run as the ring form?  (no GELU / FP8 / B-side ReLU epilogue variants there; 32-bit byte
// offsets into every operand)
bool m2f_gemm_ring_ok(const GemmBatch& gb, bool b_t) {
    for (int i = 0; i < gb.count; ++i) {
        const GemmProblem& p = gb.pr[i];
        if ((p.flags & (GF_GELU_OUT | GF_RELU_B)) || p.c8 || p.bias_grad) return false;
        if (!operands_below_2gib(p, b_t)) return false;
    }
    return true;
}

// ... and as the 256x128 ring form, whose epilogue knows bias, ReLU, GELU and a residual only?
bool m2f_gemm_ring256_ok(const GemmBatch& gb, bool b_t) {
    for (int i = 0; i < gb.count; ++i) {
        const GemmProblem& p = gb.pr[i];
        if ((p.flags & (GF_RELU_B | GF_ACCUM)) || p.c8 || p.bias_grad || p.gate || p.drop_site) return false;
        if (!operands_below_2gib(p, b_t)) return false;
    }
    return true;
}

// ... and as the eight-phase 256x256 form: that epilogue set, single segment, k a multiple of 64, no ReLU on A
bool m2f_gemm_p8_ok(const GemmBatch& gb, bool b_t) {
    if (!m2f_gemm_ring256_ok(gb, b_t)) return false;
    for (int i = 0; i < gb.count; ++i) {
        const GemmProblem& p = gb.pr[i];
        if (p.a.k[1] != 0 || p.b.k[1] != 0 || (p.a.k[0] & 63) || (p.flags & GF_RELU_A)) return false;
    }
    return true;
}

bool m2f_gemm_p8_table_ok(const std::vector<GemmProblem>& prs) {
    for (const GemmProblem& p : prs)
        if ((p.flags & GF_RELU_A) || p.a.k[1] || p.b.k[1]) return false;
    return true;
}

// ---- the chooser ---------------------------------------------------------------------------------------------------------------
namespace {

GemmChoice choice(int form, int tile_m, int tile_n) { return GemmChoice{form, tile_m, tile_n, false, false, 1}; }

// The classifier head (skinny.hip): one problem, a single segment, bias / ReLU / gate epilogue.  NT with N <= 8 (no gate) or NN with
// K <= 8, whatever M: a token row's result must not depend on how many rows the launch has - packed and padded plans agree bit for bit.
// shadows: the launch's shadow-source rule says yes; the kernels read A and B themselves, so both need their own shadow
bool choose_skinny(const GemmBatch& gb, int prec, int layout, bool shadows, GemmChoice& ch) {
    if (gb.count != 1 || (prec != M2F_PREC_BF16 && prec != M2F_PREC_F32)) return false;
    const GemmProblem& p = gb.pr[0];
    const int K = p.a.k[0];
    if (p.a.k[1] || p.b.k[1] || p.res || p.drop_site || p.c8 || p.bias_grad || !p.c || K < 1 ||
        (p.flags & (GF_ACCUM | GF_RELU_A | GF_RELU_B | GF_GELU_OUT)))
        return false;
    const bool nt = layout == M2F_LAYOUT_NT && p.N <= 8 && !p.gate;
    const bool nn = layout == M2F_LAYOUT_NN && K <= 8;
    if (!nt && !nn) return false;
    const bool use16 = shadows && p.a.q[0] && p.b.q[0];
    if (!use16 && (!p.a.p[0] || !p.b.p[0])) return false;
    auto al = [](const void* q, int a) { return (reinterpret_cast<uintptr_t>(q) & (uintptr_t)(a - 1)) == 0; };
    bool vec;
    if (nt) {       // rows of A and B in 16-byte chunks
        vec = use16 ? ((K & 7) == 0 && (p.a.ldq[0] & 7) == 0 && (p.b.ldq[0] & 7) == 0 && al(p.a.q[0], 16) && al(p.b.q[0], 16))
                    : ((K & 3) == 0 && (p.a.ld[0] & 3) == 0 && (p.b.ld[0] & 3) == 0 && al(p.a.p[0], 16) && al(p.b.p[0], 16));
    } else {        // four columns of B's rows, the gate, C (and their bf16 forms: 8 bytes)
        const uint16_t* c16 = m2f_gemm_c_shadow(gb, p.c);
        vec = (p.N & 3) == 0 && (p.ldc & 3) == 0 && al(p.c, 16) && (!c16 || al(c16, 8)) && (!p.bias || al(p.bias, 16)) &&
              (!p.gate || ((p.ldgate & 3) == 0 && al(p.gate, 16))) &&
              (use16 ? ((p.b.ldq[0] & 3) == 0 && al(p.b.q[0], 8)) : ((p.b.ld[0] & 3) == 0 && al(p.b.p[0], 16)));
    }
    ch = choice((nt ? M2F_FORM_SKINNY_NT : M2F_FORM_SKINNY_NN) | (vec ? M2F_FORM_VEC : 0) | (use16 ? M2F_FORM_SRC16 : 0), 0, 0);
    ch.src16 = use16;
    return true;
}

// bf16 mode, every operand staged from its shadow.  (a_rc, b_rc): the layout the launch RUNS in (an NN launch through B^T runs as NT)
GemmChoice choose_src16(const GemmBatch& gb, bool a_rc, bool b_rc, bool b_t, int tile) {
    const GemmKnobs& k = m2f_gemm_knobs();
    const bool auto_tile = tile == 0;
    // 128x128 tiles halve the bytes pulled per output element; used once the launch still fills the chip with them
    // (wgrad launches: measured 3.25 -> 3.18 ms/step with the threshold at 256 instead of 512)
    if (tile == 0) tile = (count_tiles(gb, 128, 128) >= (a_rc ? 256 : 512)) ? 128 : 64;
    // very large forward-form launches (the text encoder: M = utterances x tokens): 256 (M) x 128 (N) tiles, 85 instead of
    // 64 FLOP per byte through the L1 fill path that bounds these kernels
    // (RoBERTa-large geometry, 512 utterances x 64 tokens: 59.3 -> 55.7 ms per forward)
    if (tile == 128 && !a_rc && !b_rc && count_tiles(gb, 256, 128) >= 1024) tile = 256;
    if (!a_rc && !b_rc && k.ring && auto_tile) {                // the LDS-DMA forms: forward form, automatic tile only
        // eight-phase form: from p8_min tiles of 256x256, and only when those tiles fill whole rounds of the chip: a 256 x 256 tile is
        // ~25 us of work, and 336 of them on 256 CUs - the merged QKV projections of the C3 geometry at B = 256 - ran 2 % of the STEP
        // slower than three rounds of 256 x 128 ring tiles
        const int t256 = count_tiles(gb, 256, 256), rounds = (t256 + 255) / 256;
        if (k.p8 && t256 >= k.p8_min && t256 * 100 >= 85 * rounds * 256 && m2f_gemm_p8_ok(gb, b_t)) return choice(M2F_FORM_P8_KC, 256, 256);
        if (count_tiles(gb, 256, 128) >= k.ring256_min && m2f_gemm_ring256_ok(gb, b_t)) return choice(M2F_FORM_RING_256x128, 256, 128);
        // (what the 256x128 ring form cannot take - it has bias / ReLU / GELU / residual epilogues only - keeps the register-staged
        // 256x128 build from 1,024 such tiles on: RoBERTa-large geometry 52.3 vs 54.0 ms with 128x128 ring tiles)
        if (tile != 256) {
            const int t128 = count_tiles(gb, 128, 128);
            if (k.ring256_2r && t128 > 256 && t128 < 512 && count_tiles(gb, 256, 128) <= 256 && m2f_gemm_ring256_ok(gb, b_t) && m2f_gemm_ring_ok(gb, b_t))
                return choice(M2F_FORM_RING_256x128, 256, 128);           // two rounds of 128x128 tiles -> one of 256x128
            if (m2f_gemm_ring_ok(gb, b_t)) {
                if (t128 >= k.ring_min) return choice(M2F_FORM_RING_128x128, 128, 128);
                if (count_tiles(gb, 128, 64) >= k.ring64_min) return choice(M2F_FORM_RING_128x64, 128, 64);
                if (count_tiles(gb, 64, 64) >= k.ring32_min) return choice(M2F_FORM_RING_64x64, 64, 64);
            }
        }
    }
    // register-staged (gemm.hip): 256x128 (forward form), 128x128, or the one 64x64 build
    return choice(tile == 256 ? M2F_FORM_BF16SRC_256x128 : tile == 128 ? M2F_FORM_BF16SRC_128 : M2F_FORM_BF16SRC_64, tile, tile == 256 ? 128 : tile);
}

// fp32 mode, and bf16 mode with an operand that has no (usable) shadow: staged from the fp32 originals
GemmChoice choose_f32src(const GemmBatch& gb, int prec, bool a_rc, bool b_rc, int tile) {
    if (tile == 0) tile = (count_tiles(gb, 128, 128) >= 512) ? 128 : 64;     // fill 256 CUs first
    // split-K when the launch cannot occupy the chip: a CU pulls operands at a fixed ~25-45 GB/s (L1 miss queue x
    // latency), so small grids are spread over more CUs.  Only for the forward / dgrad forms on 64x64 tiles.
    const int bk = prec == M2F_PREC_F32 ? 64 : 128;             // (k-tile of the 64x64 builds)
    int want_s = 1;
    const int plain = count_tiles(gb, tile, tile);
    if (tile == 64 && !a_rc && gb.splitk_ws && gb.splitk_cnt && plain > 0 && plain < 224) {
        want_s = (352 + plain - 1) / plain;
        if (want_s > 4) want_s = 4;
        int slabs = 0;
        for (int i = 0; i < gb.count; ++i) slabs += m2f_cdiv(gb.pr[i].M, 64) * m2f_cdiv(gb.pr[i].N, 64) * m2f_gemm_splitk_of(gb.pr[i], want_s, bk);
        if (plain > gb.splitk_max_tiles || slabs > 4 * gb.splitk_max_tiles) want_s = 1;          // scratch too small: no split
    }
    bool split = false, vec = true;
    for (int i = 0; i < gb.count; ++i) {
        const GemmProblem& p = gb.pr[i];
        split = split || m2f_gemm_splitk_of(p, want_s, bk) > 1;
        vec = vec && vec_ok(p.a, a_rc, p.M) && vec_ok(p.b, b_rc, p.N);       // 16-byte loads only when every operand of every problem allows them
    }
    GemmChoice ch = choice((tile == 128 ? M2F_FORM_F32SRC_128 : split ? M2F_FORM_F32SRC_SPLITK : M2F_FORM_F32SRC_64) | (vec ? M2F_FORM_VEC : 0), tile, tile);
    ch.splitk = want_s;
    return ch;
}

}  // namespace

GemmChoice m2f_gemm_choose(const GemmBatch& gb, int prec, int layout, int tile) {
    const bool a_rc = layout == M2F_LAYOUT_TN, b_rc = layout != M2F_LAYOUT_NT;
    // dgrad against a weight whose TRANSPOSED bf16 shadow exists runs as the k-contiguous (forward) form, the
    // fastest staging path: C = A * B  ==  A * (B^T)^T
    bool b_t = prec == M2F_PREC_BF16 && layout == M2F_LAYOUT_NN;
    for (int i = 0; b_t && i < gb.count; ++i)
        for (int sgm = 0; sgm < 2; ++sgm)
            if (gb.pr[i].b.k[sgm] && !gb.pr[i].b.qt[sgm]) b_t = false;
    b_t = b_t && src16_ok(gb, false, false, true);
    const bool src16 = prec == M2F_PREC_BF16 && (b_t || src16_ok(gb, a_rc, b_rc, false));
    GemmChoice ch;
    if (m2f_gemm_knobs().skinny && choose_skinny(gb, prec, layout, src16, ch)) return ch;
    if (!src16) return choose_f32src(gb, prec, a_rc, b_rc, tile);
    ch = b_t ? choose_src16(gb, false, false, true, tile) : choose_src16(gb, a_rc, b_rc, false, tile);
    ch.src16 = true;
    ch.b_t = b_t;
    if (b_t) ch.form |= M2F_FORM_NN_T;
    return ch;
}

// fp8 (e4m3 operands, forward form, one problem); k and ldq in bytes
GemmChoice m2f_gemm_choose_fp8(const GemmBatch& gb) {
    const GemmKnobs& k = m2f_gemm_knobs();
    const GemmProblem& p = gb.pr[0];
    const bool small = (size_t)p.M * p.a.ldq[0] < 0x80000000ull && (size_t)p.N * p.b.ldq[0] < 0x80000000ull;      // 32-bit byte offsets
    // 256x256 tiles on the eight-phase schedule (gemm_p8.h, EPI 4) from one chip-filling round on, when its tiles fill whole rounds
    // (M2F_P8=0 / M2F_P8_MIN as for the bf16 launches; k a multiple of 128)
    const int t256 = m2f_cdiv(p.M, 256) * m2f_cdiv(p.N, 256), rounds = m2f_cdiv(t256, 256);
    if (k.p8 && small && t256 >= k.p8_min && t256 * 100 >= 85 * rounds * 256 && !(p.a.k[0] & 127) && (!p.c8 || (p.ldc & 7) == 0))
        return choice(M2F_FORM_FP8_P8, 256, 256);
    const int t256x128 = m2f_cdiv(p.M, 256) * m2f_cdiv(p.N, 128);
    const bool whole = p.M % 256 == 0 && p.N % 128 == 0;        // (the ring epilogue writes e4m3 results of whole tiles only)
    if (k.ring_fp8 && small && t256x128 >= 256 && !(p.flags & GF_RELU_OUT) && (!p.c8 || whole)) return choice(M2F_FORM_FP8_RING, 256, 128);
    return t256x128 < 1024 ? choice(M2F_FORM_FP8_128x128, 128, 128) : choice(M2F_FORM_FP8_256x128, 256, 128);
}

bool m2f_gemm_stages_bf16(const GemmBatch& gb, int layout) { return m2f_gemm_choose(gb, M2F_PREC_BF16, layout, 0).src16; }

// ---- the launchers: validate, choose, execute the choice -------------------------------------------------------------------------
hipError_t m2f_ring_launch_128x128(GemmBatch& gb, hipStream_t stream);
hipError_t m2f_ring_launch_128x64(GemmBatch& gb, hipStream_t stream);
hipError_t m2f_ring_launch_64x64(GemmBatch& gb, hipStream_t stream);
hipError_t m2f_ring_launch_256x128(GemmBatch& gb, hipStream_t stream);

hipError_t m2f_launch_gemm_ring(GemmBatch& gb, int bm, int bn, hipStream_t stream) {
    if (bm == 128 && bn == 128) return m2f_ring_launch_128x128(gb, stream);
    if (bm == 128 && bn == 64) return m2f_ring_launch_128x64(gb, stream);
    if (bm == 64 && bn == 64) return m2f_ring_launch_64x64(gb, stream);
    if (bm == 256 && bn == 128) return m2f_ring_launch_256x128(gb, stream);          // needs m2f_gemm_ring256_ok
    return hipErrorInvalidValue;
}

namespace {

// refuses what no kernel takes, and marks the operands the fp32-source kernels may move in 16-byte chunks
bool validate(GemmBatch& gb, int layout) {
    if (gb.count <= 0 || gb.count > M2F_GEMM_MAX_PROBLEMS) return false;
    const bool a_rc = layout == M2F_LAYOUT_TN, b_rc = layout != M2F_LAYOUT_NT;
    for (int i = 0; i < gb.count; ++i) {
        GemmProblem& p = gb.pr[i];
        if (p.a.k[0] != p.b.k[0] || p.a.k[1] != p.b.k[1] || p.M <= 0 || p.N <= 0 || p.a.k[0] <= 0) return false;
        if (p.drop_site && !gb.rng) return false;
        p.flags &= ~(uint32_t)(GF_VEC_A | GF_VEC_B);
        if (vec_ok(p.a, a_rc, p.M)) p.flags |= GF_VEC_A;
        if (vec_ok(p.b, b_rc, p.N)) p.flags |= GF_VEC_B;
    }
    return true;
}

bool validate_fp8(const GemmBatch& gb) {
    if (gb.count != 1) return false;
    const GemmProblem& p = gb.pr[0];
    return !(p.M <= 0 || p.N <= 0 || p.a.k[0] <= 0 || p.a.k[1] != 0 || p.a.k[0] != p.b.k[0] || (p.a.k[0] & 15) || !p.a.q[0] || !p.b.q[0] ||
             (p.a.ldq[0] & 15) || (p.b.ldq[0] & 15) || (reinterpret_cast<uintptr_t>(p.a.q[0]) & 15) || (reinterpret_cast<uintptr_t>(p.b.q[0]) & 15) ||
             p.gate || (p.flags & (GF_ACCUM | GF_RELU_A | GF_RELU_B)) || p.drop_site);
}

// THE site that records a dispatched launch's form (m2f_gemm_last_form)
hipError_t execute(GemmBatch& gb, const GemmChoice& ch, int prec, int layout, hipStream_t stream) {
    m2f_g_last_form = ch.form;
    switch (ch.form & 0xFF) {
        case M2F_FORM_SKINNY_NT: case M2F_FORM_SKINNY_NN: return m2f_launch_gemm_skinny(gb, ch, prec, stream);
        case M2F_FORM_P8_KC: return m2f_p8_launch_kc(gb, stream);
        case M2F_FORM_FP8_P8: return m2f_p8_launch_kc_fp8(gb, stream);
        case M2F_FORM_FP8_RING: return m2f_ring_launch_256x128_fp8(gb, stream);
        case M2F_FORM_RING_64x64: case M2F_FORM_RING_128x64: case M2F_FORM_RING_128x128: case M2F_FORM_RING_256x128:
            return m2f_launch_gemm_ring(gb, ch.tile_m, ch.tile_n, stream);
        default: return m2f_launch_gemm_staged(gb, ch, prec, layout, stream);
    }
}

}  // namespace

hipError_t m2f_launch_gemm(GemmBatch& gb, int prec, int layout, int tile, hipStream_t stream) {
    m2f_g_last_form = M2F_FORM_NONE;
    if (!validate(gb, layout)) return hipErrorInvalidValue;
    const GemmChoice ch = m2f_gemm_choose(gb, prec, layout, tile);
    if (!ch.b_t) return execute(gb, ch, prec, layout, stream);
    GemmBatch t = gb;                                           // B through its transposed shadow: the launch's own copy
    for (int i = 0; i < t.count; ++i)
        for (int sgm = 0; sgm < 2; ++sgm) { t.pr[i].b.q[sgm] = t.pr[i].b.qt[sgm]; t.pr[i].b.ldq[sgm] = t.pr[i].b.ldqt[sgm]; }
    return execute(t, ch, prec, layout, stream);
}

hipError_t m2f_launch_gemm_fp8(GemmBatch& gb, hipStream_t stream) {
    m2f_g_last_form = M2F_FORM_NONE;
    if (!validate_fp8(gb)) return hipErrorInvalidValue;
    const GemmChoice ch = m2f_gemm_choose_fp8(gb);
    // the staging code moves 16-byte chunks of a row whatever they hold: hand it the rows in byte pairs
    GemmProblem& p = gb.pr[0];
    p.a.k[0] >>= 1; p.b.k[0] >>= 1; p.a.ldq[0] >>= 1; p.b.ldq[0] >>= 1;
    return execute(gb, ch, M2F_PREC_BF16, M2F_LAYOUT_NT, stream);
}

hipError_t m2f_launch_gemm_table(const GemmBatch& gb, hipStream_t stream) {
    if (!gb.table || gb.total_tiles <= 0) return hipErrorInvalidValue;
    return gb.table_p8 ? m2f_p8_launch_table_rc(gb, stream) : m2f_ring_launch_table_rc_256x128(gb, stream);
}

hipError_t m2f_launch_gemm_table_acc(const GemmBatch& gb, hipStream_t stream) {
    if (!gb.table || gb.total_tiles <= 0) return hipErrorInvalidValue;
    return gb.table_p8 ? m2f_p8_launch_table_rc_acc(gb, stream) : m2f_ring_launch_table_rc_256x128_acc(gb, stream);
}

// ---- the tile walk of the table launches (host only; the declaration in ops.h describes the two walks) ---------------------------
int m2f_gemm_table_walk(const std::vector<GemmProblem>& prs_all, int walk, int n_wg, int tile_m, int tile_n, std::vector<uint32_t>& tile_rec, std::vector<int>& wg_begin,
                        const std::vector<int>* only) {
    const int TILE = tile_n;
    // `only` (nullable): walk just these problems (records still carry the index into prs_all = the device table)
    std::vector<size_t> sel;
    if (only) for (int i : *only) sel.push_back((size_t)i);
    else for (size_t i = 0; i < prs_all.size(); ++i) sel.push_back(i);
    struct View { const std::vector<GemmProblem>& a; const std::vector<size_t>& s; size_t size() const { return s.size(); }
                  const GemmProblem& operator[](size_t i) const { return a[s[i]]; } } prs{prs_all, sel};
    tile_rec.clear();
    wg_begin.assign((size_t)n_wg + 1, 0);
    if (n_wg < 1) return -1;
    auto rec = [&](size_t p, int mt, int nt) { return (uint32_t)sel[p] | ((uint32_t)mt << 16) | ((uint32_t)nt << 24); };
    if (prs_all.size() > 65535) return -1;
    std::vector<std::vector<uint32_t>> per_wg((size_t)n_wg);
    if (walk == 0) {
        // problem by problem, m fastest inside a problem, dealt as ring_xcd_remap deals it
        std::vector<uint32_t> all;
        for (size_t p = 0; p < prs.size(); ++p) {
            const int tm = m2f_cdiv(prs[p].M, tile_m), tn = m2f_cdiv(prs[p].N, TILE);
            if (tm > 255 || tn > 255) return -1;
            for (int nt = 0; nt < tn; ++nt)
                for (int mt = 0; mt < tm; ++mt) all.push_back(rec(p, mt, nt));
        }
        const int q = n_wg >> 3, r = n_wg & 7;
        for (int b = 0; b < n_wg; ++b) {
            const int x = b & 7, j = b >> 3;
            const int first = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
            for (size_t t = (size_t)first; t < all.size(); t += (size_t)n_wg) per_wg[(size_t)b].push_back(all[t]);
        }
    } else {
        // items = super-tiles of up to 8 (m) x 4 (n) tiles, problem-major, n-strip-major inside a problem (consecutive items
        // of a strip share their column panels); the item list is cut into eight contiguous ranges of about equal tile count
        struct Item { std::vector<uint32_t> tiles; };
        std::vector<Item> items;
        size_t total = 0;
        for (size_t p = 0; p < prs.size(); ++p) {
            const int tm = m2f_cdiv(prs[p].M, tile_m), tn = m2f_cdiv(prs[p].N, TILE);
            if (tm > 255 || tn > 255) return -1;
            const int sm = tm < 8 ? tm : 8;
            int sn = 32 / sm; if (sn < 1) sn = 1; if (sn > tn) sn = tn;
            for (int n0 = 0; n0 < tn; n0 += sn)
                for (int m0 = 0; m0 < tm; m0 += sm) {
                    Item it;
                    for (int nt = n0; nt < std::min(tn, n0 + sn); ++nt)
                        for (int mt = m0; mt < std::min(tm, m0 + sm); ++mt) it.tiles.push_back(rec(p, mt, nt));
                    total += it.tiles.size();
                    items.push_back(std::move(it));
                }
        }
        const int n_x = n_wg < 8 ? 1 : 8;
        std::vector<std::vector<uint32_t>> seq((size_t)n_x);
        size_t done = 0, i = 0;
        for (int x = 0; x < n_x; ++x) {
            const size_t target = total * (size_t)(x + 1) / (size_t)n_x;        // cumulative share after XCD x
            while (i < items.size() && (x == n_x - 1 || done + items[i].tiles.size() / 2 < target)) {
                seq[(size_t)x].insert(seq[(size_t)x].end(), items[i].tiles.begin(), items[i].tiles.end());
                done += items[i].tiles.size();
                ++i;
            }
        }
        // workgroups of XCD x: b = x, x + 8, ... ; the j-th of them takes elements j, j + per_x, ... of the XCD's sequence
        for (int x = 0; x < n_x; ++x) {
            std::vector<int> wgs;
            for (int b = x; b < n_wg; b += n_x) wgs.push_back(b);
            for (size_t t = 0; t < seq[(size_t)x].size(); ++t) per_wg[(size_t)wgs[t % wgs.size()]].push_back(seq[(size_t)x][t]);
        }
    }
    for (int b = 0; b < n_wg; ++b) {
        wg_begin[(size_t)b] = (int)tile_rec.size();
        tile_rec.insert(tile_rec.end(), per_wg[(size_t)b].begin(), per_wg[(size_t)b].end());
    }
    wg_begin[(size_t)n_wg] = (int)tile_rec.size();
    {   // every tile of every problem exactly once, whatever the order
        std::vector<uint32_t> got = tile_rec, want;
        for (size_t p = 0; p < prs.size(); ++p)
            for (int nt = 0; nt < m2f_cdiv(prs[p].N, TILE); ++nt)
                for (int mt = 0; mt < m2f_cdiv(prs[p].M, tile_m); ++mt) want.push_back(rec(p, mt, nt));
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        if (got != want) return -1;
    }
    return (int)tile_rec.size();
}

// ---- the dry entry ---------------------------------------------------------------------------------------------------------------
// The chooser's answer for `count` identical, well-formed problems, nothing launched (include/m2fnet_hip.h).  Operand addresses are
// aligned fakes that nothing dereferences; every leading dimension is pad8 of the contiguous extent (+ 1: M2F_GEMM_FORM_ODD_LD).
extern "C" int m2f_gemm_form(int mode, int layout, int tile, int count, int M, int N, int K0, int K1, uint32_t bits, int* stages_bf16) {
    if (stages_bf16) *stages_bf16 = 0;
    if (mode < 0 || mode > 2 || layout < M2F_LAYOUT_NT || layout > M2F_LAYOUT_TN || count < 1 || count > M2F_GEMM_MAX_PROBLEMS) return M2F_FORM_NONE;
    const bool fp8 = mode == 2;
    const bool a_rc = layout == M2F_LAYOUT_TN, b_rc = layout != M2F_LAYOUT_NT;
    const int odd = (bits & M2F_GEMM_FORM_ODD_LD) ? 1 : 0;
    auto ld_of = [&](int extent) { return ((extent + 7) & ~7) + odd; };
    uintptr_t next = 0x100000;                                  // fake addresses: 256-byte aligned, 4 GiB apart, never dereferenced
    auto fake = [&]() { next += 0x100000000ull; return next; };
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    const int k[2] = {K0, K1};
    for (int i = 0; i < count; ++i) {
        GemmProblem& p = gb.pr[i];
        p.M = M; p.N = N;
        for (int s = 0; s < 2 && k[s] > 0; ++s) {
            p.a.k[s] = p.b.k[s] = k[s];
            if (fp8) {                                          // e4m3 bytes behind q, as m2f_gemm_fp8 passes them
                p.a.q[s] = reinterpret_cast<const uint16_t*>(fake()); p.b.q[s] = reinterpret_cast<const uint16_t*>(fake());
                p.a.ldq[s] = p.b.ldq[s] = ld_of(k[s]);
                continue;
            }
            p.a.p[s] = reinterpret_cast<const float*>(fake()); p.b.p[s] = reinterpret_cast<const float*>(fake());
            p.a.ld[s] = ld_of(a_rc ? M : k[s]); p.b.ld[s] = ld_of(b_rc ? N : k[s]);
            if (bits & M2F_GEMM_FORM_SHADOWS) {
                p.a.q[s] = reinterpret_cast<const uint16_t*>(fake()); p.b.q[s] = reinterpret_cast<const uint16_t*>(fake());
                p.a.ldq[s] = p.a.ld[s]; p.b.ldq[s] = p.b.ld[s];
            }
            if (bits & M2F_GEMM_FORM_BT_SHADOW) { p.b.qt[s] = reinterpret_cast<const uint16_t*>(fake()); p.b.ldqt[s] = ld_of(k[s]); }
        }
        p.ldc = ld_of(N); p.gate_scale = 1.f; p.acc_scale = 1.f;
        if (bits & M2F_GEMM_FORM_C8) { p.c8 = reinterpret_cast<uint8_t*>(fake()); p.c8_scale = 1.f; }
        else p.c = reinterpret_cast<float*>(fake());
        if (bits & M2F_GEMM_FORM_RES) { p.res = reinterpret_cast<const float*>(fake()); p.ldres = ld_of(N); }
        if (bits & M2F_GEMM_FORM_GATE) { p.gate = reinterpret_cast<const float*>(fake()); p.ldgate = ld_of(N); }
        if (bits & M2F_GEMM_FORM_BIAS_GRAD) p.bias_grad = reinterpret_cast<float*>(fake());
        if (bits & M2F_GEMM_FORM_DROP) p.drop_site = 7;
        p.flags = ((bits & M2F_GEMM_FORM_RELU_A) ? GF_RELU_A : 0) | ((bits & M2F_GEMM_FORM_RELU_B) ? GF_RELU_B : 0) |
                  ((bits & M2F_GEMM_FORM_RELU_OUT) ? GF_RELU_OUT : 0) | ((bits & M2F_GEMM_FORM_GELU) ? GF_GELU_OUT : 0) |
                  ((bits & M2F_GEMM_FORM_ACC) ? GF_ACCUM : 0);
    }
    gb.count = count;
    if (bits & M2F_GEMM_FORM_DROP) { gb.rng = reinterpret_cast<const uint32_t*>(fake()); gb.drop_scale = 2.f; gb.drop_thresh = 0x80000000u; }
    if (bits & M2F_GEMM_FORM_SPLITK) {
        gb.splitk_ws = reinterpret_cast<float*>(fake()); gb.splitk_cnt = reinterpret_cast<unsigned*>(fake()); gb.splitk_max_tiles = M2F_SPLITK_MAX_TILES;
    }
    if (fp8) return validate_fp8(gb) ? m2f_gemm_choose_fp8(gb).form : M2F_FORM_NONE;
    if (!validate(gb, layout)) return M2F_FORM_NONE;
    if (stages_bf16) *stages_bf16 = m2f_gemm_stages_bf16(gb, layout) ? 1 : 0;
    return m2f_gemm_choose(gb, mode, layout, tile).form;
}
