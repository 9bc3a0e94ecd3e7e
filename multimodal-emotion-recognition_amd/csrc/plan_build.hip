// The launch-list builder of a plan (plan.h; the decisions behind the lists: top of plan.hip): build_plan lays the workspace out and writes
// m2f_plan::built, and the two walks over finished lists that the switches of plan.hip need (build_accumulate, table_coverage).
#include "plan.h"

using namespace m2f;

namespace {

Op op_gemm(int layout, const GemmProblem& p) { Op o; o.kind = OP_GEMM; o.layout = layout; o.gp.push_back(p); return o; }

struct Builder {
    m2f_plan& P;
    Arena ar;
    uint32_t next_site = 1;
    std::vector<Op> chain_f;                   // sequential forward ops after the branches (FAM, classifier)
    std::vector<Op> br_f[2], br_b[2];          // per-branch (0 audio, 1 text) forward / backward chains
    std::vector<Op> chain_b;                   // classifier + FAM backward (before the branches)
    std::vector<Op> in_b[2];                   // per-branch input-gradient launches (m2f_plan_backward_outputs), after the branches
    std::vector<GemmProblem> wgrads;           // deferred weight-gradient problems (TN)
    std::vector<std::pair<int, int>> wdeps;    // per wgrad problem: (chain id, index) of the last op emitted before it
    int cur_chain = 2;                         // chain being built: 0 audio branch, 1 text branch, 2 head (chain_b)
    std::vector<LnReduceItem> lnitems;
    ModBuf mod[2];
    std::vector<FamBuf> fam;
    int T;

    explicit Builder(m2f_plan& p) : P(p), T(p.T) {}

    static int pad8(int w) { return (w + 7) & ~7; }     // activation leading dimensions: multiples of 8 (bf16 shadows stay 16-byte aligned)
    uint32_t site() { return P.use_dropout ? next_site++ : 0u; }
    const float* W(size_t off) const { return P.params + off; }
    float* G(size_t off) const { return P.grads ? P.grads + off : nullptr; }
    float gscale() const { return P.use_dropout ? P.drop_scale : 1.f; }

    Op op_ln_fwd(const float* x, size_t gw, size_t gb, const float* res, float* out, float* stats, int d, int ld, uint32_t s) {
        Op o; o.kind = OP_LN_FWD;
        LnProblem p; memset(&p, 0, sizeof(p));
        p.x = x; p.gamma = W(gw); p.beta = W(gb); p.res = res; p.out = out; p.stats = stats; p.d = d; p.ld = ld; p.drop_site = s;
        o.lp.push_back(p);
        return o;
    }
    // shared_partial != null: the LayerNorm object is shared (final encoder norm): the caller owns one partial
    // buffer for all its uses and registers a single reduce item covering every slice.
    Op op_ln_bwd(const float* x, size_t gw, size_t gb, const float* stats, const float* dy, const float* extra,
                 float* dx, float* dx_masked, int d, int ld, uint32_t s2, float* shared_partial = nullptr) {
        Op o; o.kind = OP_LN_BWD;
        LnProblem p; memset(&p, 0, sizeof(p));
        p.x = x; p.gamma = W(gw); p.stats = const_cast<float*>(stats); p.dy = dy; p.extra = extra; p.dx = dx;
        p.dx_masked = dx_masked; p.d = d; p.ld = ld; p.drop_site2 = s2;
        const int nblk = m2f_ln_row_blocks(T);
        p.partial = shared_partial ? shared_partial : ar.f((size_t)nblk * 2 * d);
        o.lp.push_back(p);
        if (!shared_partial && P.param_grads) {
            LnReduceItem it; it.partial = p.partial; it.dgamma = G(gw); it.dbeta = G(gb); it.d = d; it.nblk = nblk;
            lnitems.push_back(it);
        }
        return o;
    }
    void wgrad(const float* dy, int lddy, const float* x, int ldx, int Nw, int Kw, size_t w_off, int ldw, long b_off,
               bool relu_b = false) {
        // dW[Nw, Kw] = dY[T, Nw]^T X[T, Kw]; bias grad = column sums of dY
        if (!P.param_grads) return;              // input gradients only (m2f_plan_backward_outputs)
        GemmProblem p = gp_make(dy, lddy, x, ldx, Nw, Kw, T, G(w_off), ldw);
        if (b_off >= 0) p.bias_grad = G((size_t)b_off);
        if (relu_b) p.flags |= GF_RELU_B;
        wgrads.push_back(p);
        const std::vector<Op>& cur = cur_chain == 2 ? chain_b : br_b[cur_chain];
        wdeps.push_back({cur_chain, (int)cur.size() - 1});
    }

    // ---------------- modality branch: encoders + projection --------------------------------------
    void build_modality(int bi, const ModalityP& mp, int d, int H, int nl, int nt, const float* x_in) {
        ModBuf& m = mod[bi];
        m.d = d; m.H = H; m.nl = nl; m.nt = nt; m.x_in = x_in;
        const int F = P.cfg.dim_ff, E = P.cfg.d_fam;
        const int dp = pad8(d), d3p = pad8(3 * d), Fp = pad8(F), Ep = pad8(E);   // activation leading dimensions
        std::vector<Op>& f = br_f[bi];
        const float* x = x_in;
        m.L.resize(nt);
        for (int e = 0; e < nt; ++e) {
            const float* y = x;
            for (int l = 0; l < nl; ++l) {
                const EncLayerP& p = mp.enc[e][l];
                EncLayerBuf b;
                b.y_in = y;
                b.qkv = ar.f((size_t)T * d3p);
                b.probs = ar.f(m2f_attn_probs_elems(P.B, H, P.L));
                b.att = ar.f((size_t)T * dp);
                b.s1 = ar.f((size_t)T * dp);
                b.st1 = ar.f((size_t)T * 2);
                b.y1 = ar.f((size_t)T * dp);
                b.h = ar.f((size_t)T * Fp);
                b.s2 = ar.f((size_t)T * dp);
                b.st2 = ar.f((size_t)T * 2);
                b.y2 = ar.f((size_t)T * dp);
                b.site_attn = site(); b.site_d1 = site(); b.site_ff = site(); b.site_d2 = site();
                {   // packed QKV in-projection
                    GemmProblem g = gp_make(y, dp, W(p.in_w), d, T, 3 * d, d, b.qkv, d3p);
                    g.bias = W(p.in_b);
                    f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                {
                    Op o; o.kind = OP_ATTN_FWD;
                    AttnProblem a; memset(&a, 0, sizeof(a));
                    a.q = b.qkv; a.k = b.qkv + d; a.v = b.qkv + 2 * d; a.ldq = a.ldk = a.ldv = d3p;
                    a.out = b.att; a.ldo = dp; a.probs = b.probs; a.H = H; a.hd = d / H; a.drop_site = b.site_attn;
                    o.ap.push_back(a);
                    f.push_back(o);
                }
                {   // out-proj -> dropout1 -> + residual
                    GemmProblem g = gp_make(b.att, dp, W(p.out_w), d, T, d, d, b.s1, dp);
                    g.bias = W(p.out_b); g.drop_site = b.site_d1; g.res = y; g.ldres = dp;
                    f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                f.push_back(op_ln_fwd(b.s1, p.n1_w, p.n1_b, nullptr, b.y1, b.st1, d, dp, 0));
                {   // linear1 -> relu -> dropout
                    GemmProblem g = gp_make(b.y1, dp, W(p.l1_w), d, T, F, d, b.h, Fp);
                    g.bias = W(p.l1_b); g.flags |= GF_RELU_OUT; g.drop_site = b.site_ff;
                    f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                {   // linear2 -> dropout2 -> + residual
                    GemmProblem g = gp_make(b.h, Fp, W(p.l2_w), F, T, d, F, b.s2, dp);
                    g.bias = W(p.l2_b); g.drop_site = b.site_d2; g.res = b.y1; g.ldres = dp;
                    f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                f.push_back(op_ln_fwd(b.s2, p.n2_w, p.n2_b, nullptr, b.y2, b.st2, d, dp, 0));
                y = b.y2;
                m.L[e].push_back(b);
            }
            // x_e = x_{e-1} + LNf(y); the last one feeds `dropout -> proj` (src/model.py:111,123)
            float* xe = ar.f((size_t)T * dp);
            float* stf = ar.f((size_t)T * 2);
            const uint32_t s = (e == nt - 1) ? (m.site_pre = site()) : 0u;
            f.push_back(op_ln_fwd(y, mp.norm_w, mp.norm_b, x, xe, stf, d, dp, s));
            m.xe.push_back(xe);
            m.stf.push_back(stf);
            x = xe;
        }
        m.xp = ar.f((size_t)T * Ep);
        m.site_post = site();
        {
            GemmProblem g = gp_make(x, dp, W(mp.proj_w), d, T, E, d, m.xp, Ep);
            g.bias = W(mp.proj_b); g.drop_site = m.site_post;
            f.push_back(op_gemm(M2F_LAYOUT_NT, g));
        }
    }

    // backward of a modality branch given d(xp) (already masked by the post-proj dropout).  With the modality's bit in
    // P.in_mask the chain runs on to d x_in (reference src/model.py:106-119: x_in feeds encoder stack 0 and, through the outer
    // skip x + enc(x), its output) and leaves it in M2F_BUF_DTEXT / M2F_BUF_DAUDIO.  The launches that only the input gradient
    // needs go to in_b[bi], appended behind the merged branch chains, so the launches of the default backward and their
    // grouping stay exactly as they are; the arena holds the same buffers whatever the setting (one workspace size).
    void build_modality_bwd(int bi, const ModalityP& mp, const float* dxp) {
        ModBuf& m = mod[bi];
        const int d = m.d, H = m.H, nl = m.nl, nt = m.nt, F = P.cfg.dim_ff, E = P.cfg.d_fam;
        const int dp = pad8(d), d3p = pad8(3 * d), Fp = pad8(F), Ep = pad8(E);
        std::vector<Op>& bw = br_b[bi];
        const int saved_chain = cur_chain;
        const bool want_in = (P.in_mask & (bi == 0 ? 2 : 1)) != 0;
        float* dx_in = static_cast<float*>(P.bufs[bi == 0 ? M2F_BUF_DAUDIO : M2F_BUF_DTEXT]);
        cur_chain = 2;      // the projection wgrad reads d(xp), produced by the head chain (everything emitted so far)
        const float* x_last = nt > 0 ? m.xe[nt - 1] : m.x_in;
        wgrad(dxp, Ep, x_last, dp, E, d, mp.proj_w, d, (long)mp.proj_b);
        cur_chain = bi;
        if (nt == 0) {      // no encoder stack: d x_in = d(xp) W_proj (through the pre-projection dropout)
            if (want_in) {
                GemmProblem g = gp_make(dxp, Ep, W(mp.proj_w), d, T, d, E, dx_in, dp);
                g.drop_site = m.site_pre;
                in_b[bi].push_back(op_gemm(M2F_LAYOUT_NN, g));
            }
            cur_chain = saved_chain;
            return;
        }
        float* dx = ar.f((size_t)T * dp);
        {
            GemmProblem g = gp_make(dxp, Ep, W(mp.proj_w), d, T, d, E, dx, dp);
            g.drop_site = m.site_pre;
            bw.push_back(op_gemm(M2F_LAYOUT_NN, g));
        }
        const float* dxe = dx;
        const int nblk = m2f_ln_row_blocks(T);
        float* normp = ar.f((size_t)nt * nblk * 2 * d);       // one slice per use of the shared final norm
        if (P.param_grads) {
            LnReduceItem it; it.partial = normp; it.dgamma = G(mp.norm_w); it.dbeta = G(mp.norm_b); it.d = d; it.nblk = nt * nblk;
            lnitems.push_back(it);
        }
        for (int e = nt - 1; e >= 0; --e) {
            const bool need_in = e > 0 || want_in;   // gradient w.r.t. this encoder's input is needed
            const float* yN = nl > 0 ? m.L[e][nl - 1].y2 : (e > 0 ? m.xe[e - 1] : m.x_in);
            float* g_cur = ar.f((size_t)T * dp);
            bw.push_back(op_ln_bwd(yN, mp.norm_w, mp.norm_b, m.stf[e], dxe, nullptr, g_cur, nullptr, d, dp, 0,
                                   normp + (size_t)e * nblk * 2 * d));
            const float* gy = g_cur;
            for (int l = nl - 1; l >= 0; --l) {
                const EncLayerP& p = mp.enc[e][l];
                const EncLayerBuf& b = m.L[e][l];
                const bool first = (l == 0);
                // LN2
                float* ds2 = ar.f((size_t)T * dp);
                float* ds2m = b.site_d2 ? ar.f((size_t)T * dp) : nullptr;
                bw.push_back(op_ln_bwd(b.s2, p.n2_w, p.n2_b, b.st2, gy, nullptr, ds2, ds2m, d, dp, b.site_d2));
                const float* ds2g = ds2m ? ds2m : ds2;
                wgrad(ds2g, dp, b.h, Fp, d, F, p.l2_w, F, (long)p.l2_b);
                float* dh = ar.f((size_t)T * Fp);
                {
                    GemmProblem g = gp_make(ds2g, dp, W(p.l2_w), F, T, F, d, dh, Fp);
                    g.gate = b.h; g.ldgate = Fp; g.gate_scale = b.site_ff ? P.drop_scale : 1.f;
                    bw.push_back(op_gemm(M2F_LAYOUT_NN, g));
                }
                wgrad(dh, Fp, b.y1, dp, F, d, p.l1_w, d, (long)p.l1_b);
                float* dy1 = ar.f((size_t)T * dp);
                {
                    GemmProblem g = gp_make(dh, Fp, W(p.l1_w), d, T, d, F, dy1, dp);
                    g.res = ds2; g.ldres = dp;
                    bw.push_back(op_gemm(M2F_LAYOUT_NN, g));
                }
                // LN1 (+ the encoder-level residual d x_{e-1} += d x_e on the first layer)
                const float* extra = (first && need_in) ? dxe : nullptr;
                float* ds1 = ar.f((size_t)T * dp);
                // (the masked copy is reserved on the first layer of stack 0 whatever the setting: one arena layout)
                float* ds1m = (b.site_d1 || (first && e == 0) || extra) ? ar.f((size_t)T * dp) : nullptr;
                if (!b.site_d1 && !extra) ds1m = nullptr;
                bw.push_back(op_ln_bwd(b.s1, p.n1_w, p.n1_b, b.st1, dy1, extra, ds1, ds1m, d, dp, b.site_d1));
                const float* ds1g = ds1m ? ds1m : ds1;
                wgrad(ds1g, dp, b.att, dp, d, d, p.out_w, d, (long)p.out_b);
                float* datt = ar.f((size_t)T * dp);
                bw.push_back(op_gemm(M2F_LAYOUT_NN, gp_make(ds1g, dp, W(p.out_w), d, T, d, d, datt, dp)));
                float* dqkv = ar.f((size_t)T * d3p);
                {
                    Op o; o.kind = OP_ATTN_BWD;
                    AttnProblem a; memset(&a, 0, sizeof(a));
                    a.q = b.qkv; a.k = b.qkv + d; a.v = b.qkv + 2 * d; a.ldq = a.ldk = a.ldv = d3p;
                    a.out = b.att; a.ldo = dp; a.probs = b.probs; a.H = H; a.hd = d / H; a.drop_site = b.site_attn;
                    a.dout = datt; a.lddo = dp;
                    a.dq = dqkv; a.dk = dqkv + d; a.dv = dqkv + 2 * d; a.lddq = a.lddk = a.lddv = d3p;
                    o.ap.push_back(a);
                    bw.push_back(o);
                }
                wgrad(dqkv, d3p, b.y_in, dp, 3 * d, d, p.in_w, d, (long)p.in_b);
                if (!first || need_in) {
                    const bool to_input = first && e == 0;           // d x_in itself: a launch of in_b
                    float* gn = to_input ? dx_in : ar.f((size_t)T * dp);
                    GemmProblem g = gp_make(dqkv, d3p, W(p.in_w), d, T, d, 3 * d, gn, dp);
                    g.res = ds1; g.ldres = dp;            // ds1 already carries the encoder-level residual
                    (to_input ? in_b[bi] : bw).push_back(op_gemm(M2F_LAYOUT_NN, g));
                    gy = gn;
                }
            }
            dxe = gy;
        }
        cur_chain = saved_chain;
    }

    // ---------------- fusion stack + classifier ------------------------------------------------------
    void build_head() {
        const m2f_config& c = P.cfg;
        const int E = c.d_fam, Hf = c.nhead_fam;
        const int Ep = pad8(E), E2p = pad8(2 * E);
        const bool a_on = c.audio_enabled, t_on = c.text_enabled;
        const float* a = a_on ? mod[0].xp : nullptr;
        const float* t = t_on ? mod[1].xp : nullptr;
        if (c.fam_enabled) {
            // all K projections read the same (layer-invariant) audio tensor: one grouped launch per 8 layers
            std::vector<float*> kbuf;
            for (int i = 0; i < c.nlayers_fam; ++i) kbuf.push_back(ar.f((size_t)T * Ep));
            for (int i0 = 0; i0 < c.nlayers_fam; i0 += M2F_GEMM_MAX_PROBLEMS) {
                Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_NT;
                for (int i = i0; i < std::min(c.nlayers_fam, i0 + M2F_GEMM_MAX_PROBLEMS); ++i) {
                    const FamP& p = P.pm.fam[i];
                    GemmProblem g = gp_make(a, Ep, W(p.in_w + (size_t)E * E), E, T, E, E, kbuf[i], Ep);
                    g.bias = W(p.in_b + E);
                    o.gp.push_back(g);
                }
                chain_f.push_back(o);
            }
            for (int i = 0; i < c.nlayers_fam; ++i) {
                const FamP& p = P.pm.fam[i];
                FamBuf b;
                b.t_in = t;
                b.qv = ar.f((size_t)T * E2p);
                b.k = kbuf[i];
                b.probs = ar.f(m2f_attn_probs_elems(P.B, Hf, P.L));
                b.att = ar.f((size_t)T * Ep);
                b.x = ar.f((size_t)T * Ep);
                b.t_out = ar.f((size_t)T * Ep);
                b.site_attn = site(); b.site_out = site();
                {   // q = t Wq^T + bq -> qv[:, :E] ; v = t Wv^T + bv -> qv[:, E:]
                    Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_NT;
                    GemmProblem gq = gp_make(t, Ep, W(p.in_w), E, T, E, E, b.qv, E2p);
                    gq.bias = W(p.in_b);
                    GemmProblem gv = gp_make(t, Ep, W(p.in_w + (size_t)2 * E * E), E, T, E, E, b.qv + E, E2p);
                    gv.bias = W(p.in_b + 2 * E);
                    o.gp.push_back(gq); o.gp.push_back(gv);
                    chain_f.push_back(o);
                }
                {
                    Op o; o.kind = OP_ATTN_FWD;
                    AttnProblem at; memset(&at, 0, sizeof(at));
                    at.q = b.qv; at.ldq = E2p; at.k = b.k; at.ldk = Ep; at.v = b.qv + E; at.ldv = E2p;
                    at.out = b.att; at.ldo = Ep; at.probs = b.probs; at.H = Hf; at.hd = E / Hf; at.drop_site = b.site_attn;
                    o.ap.push_back(at);
                    chain_f.push_back(o);
                }
                {
                    GemmProblem g = gp_make(b.att, Ep, W(p.out_w), E, T, E, E, b.x, Ep);
                    g.bias = W(p.out_b);
                    chain_f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                {   // relu(Linear(relu(cat(x, t)))) -> dropout   (src/model.py:16-19,131)
                    GemmProblem g = gp_make(b.x, Ep, W(p.lin_w), 2 * E, T, E, E, b.t_out, Ep);
                    gp_seg2(g, t, Ep, W(p.lin_w) + E, 2 * E, E);
                    g.bias = W(p.lin_b); g.flags |= GF_RELU_A | GF_RELU_OUT; g.drop_site = b.site_out;
                    chain_f.push_back(op_gemm(M2F_LAYOUT_NT, g));
                }
                t = b.t_out;
                fam.push_back(b);
            }
            P.bufs[M2F_BUF_FAM0_OUT] = fam.empty() ? nullptr : fam[0].t_out;
        }
        for (Op& o : chain_f) o.group = 1;                  // everything so far = the fusion stack
        const size_t cls_f0 = chain_f.size();
        // classifier (src/model.py:89-100,143): Linear0, [ReLU, Linear]*(n-2), ReLU, Dropout, Linear
        const int hid = c.cls_hidden, C = c.cls_out;
        const int hidp = pad8(hid);
        const int nhid = (int)P.pm.cls.size() - 1;           // hidden activations h[0..nhid-1]
        std::vector<float*> hbuf;
        std::vector<uint32_t> hsite;
        const float* s0 = (a_on && t_on) ? a : (t_on ? t : a);
        const float* s1 = (a_on && t_on) ? t : nullptr;
        for (int j = 0; j < nhid; ++j) {
            float* h = ar.f((size_t)T * hidp);
            const uint32_t s = (j == nhid - 1) ? site() : 0u;
            const LinP& lp = P.pm.cls[j];
            GemmProblem g;
            if (j == 0) {
                const int ldw = cls_in_width(c);
                g = gp_make(s0, Ep, W(lp.w), ldw, T, hid, E, h, hidp);
                if (s1) gp_seg2(g, s1, Ep, W(lp.w) + E, ldw, E);
            } else {
                g = gp_make(hbuf[j - 1], hidp, W(lp.w), hid, T, hid, hid, h, hidp);
            }
            g.bias = W(lp.b); g.flags |= GF_RELU_OUT; g.drop_site = s;
            chain_f.push_back(op_gemm(M2F_LAYOUT_NT, g));
            hbuf.push_back(h);
            hsite.push_back(s);
        }
        float* logits = ar.f((size_t)T * C);
        P.bufs[M2F_BUF_LOGITS] = logits;
        P.bufs[M2F_BUF_FEATURES] = hbuf[nhid - 1];
        {
            const LinP& lp = P.pm.cls[nhid];
            GemmProblem g = gp_make(hbuf[nhid - 1], hidp, W(lp.w), hid, T, C, hid, logits, C);
            g.bias = W(lp.b);
            chain_f.push_back(op_gemm(M2F_LAYOUT_NT, g));
        }
        for (size_t i = cls_f0; i < chain_f.size(); ++i) chain_f[i].group = 2;
        float* dlogits = ar.f((size_t)T * C);
        P.bufs[M2F_BUF_DLOGITS] = dlogits;
        P.loss_terms = ar.f((size_t)T * 2);
        // train plans keep (loss, den, num) in the TAIL of the flat gradient buffer, so the data-parallel all-reduce
        // carries the denominators along with the gradients and nothing has to be copied
        {
            float* ws_loss = ar.f(4);
            P.bufs[M2F_BUF_LOSS] = (P.train && P.grads) ? P.grads + P.pm.total : ws_loss;
        }
        if (!P.train) return;

        // ------------------------------ backward -----------------------------------------------------
        const float gs = gscale();
        {   // last linear
            const LinP& lp = P.pm.cls[nhid];
            wgrad(dlogits, C, hbuf[nhid - 1], hidp, C, hid, lp.w, hid, (long)lp.b);
        }
        float* dh = ar.f((size_t)T * hidp);
        {
            const LinP& lp = P.pm.cls[nhid];
            GemmProblem g = gp_make(dlogits, C, W(lp.w), hid, T, hid, C, dh, hidp);
            g.gate = hbuf[nhid - 1]; g.ldgate = hidp; g.gate_scale = hsite[nhid - 1] ? gs : 1.f;
            chain_b.push_back(op_gemm(M2F_LAYOUT_NN, g));
            // (m2f_plan_supcon adds its gradient to this launch's output, the first of the backward list, under the same gate)
            P.crit.supcon_dh = dh; P.crit.supcon_gate = g.gate_scale;
        }
        for (int j = nhid - 1; j >= 1; --j) {
            const LinP& lp = P.pm.cls[j];
            wgrad(dh, hidp, hbuf[j - 1], hidp, hid, hid, lp.w, hid, (long)lp.b);
            float* dprev = ar.f((size_t)T * hidp);
            GemmProblem g = gp_make(dh, hidp, W(lp.w), hid, T, hid, hid, dprev, hidp);
            g.gate = hbuf[j - 1]; g.ldgate = hidp; g.gate_scale = 1.f;
            chain_b.push_back(op_gemm(M2F_LAYOUT_NN, g));
            dh = dprev;
        }
        // Linear0: input = cat(a, t) | t | a
        const LinP& l0 = P.pm.cls[0];
        const int ldw0 = cls_in_width(c);
        float* d_a = a_on ? ar.f((size_t)T * Ep) : nullptr;
        float* d_t = t_on ? ar.f((size_t)T * Ep) : nullptr;
        {
            Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_NN;
            if (a_on && t_on) {
                wgrad(dh, hidp, a, Ep, hid, E, l0.w, ldw0, (long)l0.b);
                wgrad(dh, hidp, t, Ep, hid, E, l0.w + E, ldw0, -1);
                o.gp.push_back(gp_make(dh, hidp, W(l0.w), ldw0, T, E, hid, d_a, Ep));
                GemmProblem g = gp_make(dh, hidp, W(l0.w) + E, ldw0, T, E, hid, d_t, Ep);
                if (c.fam_enabled) { g.gate = t; g.ldgate = Ep; g.gate_scale = fam.back().site_out ? gs : 1.f; }
                o.gp.push_back(g);
            } else {
                const float* x = t_on ? t : a;
                float* dx = t_on ? d_t : d_a;
                wgrad(dh, hidp, x, Ep, hid, E, l0.w, ldw0, (long)l0.b);
                o.gp.push_back(gp_make(dh, hidp, W(l0.w), ldw0, T, E, hid, dx, Ep));
            }
            chain_b.push_back(o);
        }
        for (Op& o : chain_b) o.group = 2;                  // classifier backward
        const size_t fam_b0 = chain_b.size();
        // fusion layers, last to first.  `dz` = gradient w.r.t. the pre-ReLU output of layer i (the
        // ReLU/dropout gate was applied by the producer's epilogue).
        const float* dz = d_t;
        for (int i = (int)fam.size() - 1; i >= 0; --i) {
            const FamP& p = P.pm.fam[i];
            const FamBuf& b = fam[i];
            wgrad(dz, Ep, b.x, Ep, E, E, p.lin_w, 2 * E, (long)p.lin_b, true);
            wgrad(dz, Ep, b.t_in, Ep, E, E, p.lin_w + E, 2 * E, -1, true);
            float* dx = ar.f((size_t)T * Ep);
            float* dtA = ar.f((size_t)T * Ep);
            {
                Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_NN;
                GemmProblem g1 = gp_make(dz, Ep, W(p.lin_w), 2 * E, T, E, E, dx, Ep);
                g1.gate = b.x; g1.ldgate = Ep;
                GemmProblem g2 = gp_make(dz, Ep, W(p.lin_w) + E, 2 * E, T, E, E, dtA, Ep);
                g2.gate = b.t_in; g2.ldgate = Ep;
                o.gp.push_back(g1); o.gp.push_back(g2);
                chain_b.push_back(o);
            }
            wgrad(dx, Ep, b.att, Ep, E, E, p.out_w, E, (long)p.out_b);
            float* datt = ar.f((size_t)T * Ep);
            chain_b.push_back(op_gemm(M2F_LAYOUT_NN, gp_make(dx, Ep, W(p.out_w), E, T, E, E, datt, Ep)));
            float* dqv = ar.f((size_t)T * E2p);
            float* dk = ar.f((size_t)T * Ep);
            {
                Op o; o.kind = OP_ATTN_BWD;
                AttnProblem at; memset(&at, 0, sizeof(at));
                at.q = b.qv; at.ldq = E2p; at.k = b.k; at.ldk = Ep; at.v = b.qv + E; at.ldv = E2p;
                at.out = b.att; at.ldo = Ep; at.probs = b.probs; at.H = Hf; at.hd = E / Hf; at.drop_site = b.site_attn;
                at.dout = datt; at.lddo = Ep;
                at.dq = dqv; at.lddq = E2p; at.dv = dqv + E; at.lddv = E2p; at.dk = dk; at.lddk = Ep;
                o.ap.push_back(at);
                chain_b.push_back(o);
            }
            wgrad(dqv, E2p, b.t_in, Ep, E, E, p.in_w, E, (long)p.in_b);                                         // dWq, dbq
            wgrad(dk, Ep, a, Ep, E, E, p.in_w + (size_t)E * E, E, (long)(p.in_b + E));                          // dWk, dbk
            wgrad(dqv + E, E2p, b.t_in, Ep, E, E, p.in_w + (size_t)2 * E * E, E, (long)(p.in_b + 2 * E));       // dWv, dbv
            float* dt = ar.f((size_t)T * Ep);
            {
                Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_NN;
                // d t_in = dq Wq + dv Wv + dtA   (then the previous layer's ReLU/dropout gate)
                GemmProblem g = gp_make(dqv, E2p, W(p.in_w), E, T, E, E, dt, Ep);
                gp_seg2(g, dqv + E, E2p, W(p.in_w + (size_t)2 * E * E), E, E);
                g.res = dtA; g.ldres = Ep;
                if (i > 0) { g.gate = b.t_in; g.ldgate = Ep; g.gate_scale = fam[i - 1].site_out ? gs : 1.f; }
                // d audio += dk Wk
                GemmProblem ga = gp_make(dk, Ep, W(p.in_w + (size_t)E * E), E, T, E, E, d_a, Ep);
                ga.flags |= GF_ACCUM;
                o.gp.push_back(g); o.gp.push_back(ga);
                chain_b.push_back(o);
            }
            dz = dt;
        }
        d_t = const_cast<float*>(dz);
        for (size_t i = fam_b0; i < chain_b.size(); ++i) chain_b[i].group = 1;
        // gradient through the post-projection dropout (src/model.py:113,125)
        for (int bi = 0; bi < 2; ++bi) {
            float* dxp = bi == 0 ? d_a : d_t;
            if (!dxp) continue;
            if (mod[bi].site_post) {
                Op o; o.kind = OP_DROPOUT; o.dptr = dxp; o.dT = T; o.dd = E; o.dld = Ep; o.dsite = mod[bi].site_post;
                chain_b.push_back(o);
            }
            build_modality_bwd(bi, bi == 0 ? P.pm.audio : P.pm.text, dxp);
        }
    }
};

// ---- merge two independent op chains into grouped launches (LCS on compatibility) -------------------
bool compatible(const Op& a, const Op& b) {
    if (a.kind != b.kind) return false;
    switch (a.kind) {
        case OP_GEMM: return a.layout == b.layout && a.gp.size() + b.gp.size() <= M2F_GEMM_MAX_PROBLEMS;
        case OP_ATTN_FWD: case OP_ATTN_BWD: return a.ap.size() + b.ap.size() <= M2F_ATTN_MAX_PROBLEMS;
        case OP_LN_FWD: case OP_LN_BWD: return a.lp.size() + b.lp.size() <= M2F_LN_MAX_PROBLEMS;
        default: return false;
    }
}
Op merged(const Op& a, const Op& b) {
    Op o = a;
    o.src.insert(o.src.end(), b.src.begin(), b.src.end());
    o.gp.insert(o.gp.end(), b.gp.begin(), b.gp.end());
    o.ap.insert(o.ap.end(), b.ap.begin(), b.ap.end());
    o.lp.insert(o.lp.end(), b.lp.begin(), b.lp.end());
    return o;
}
std::vector<Op> merge_chains(const std::vector<Op>& A, const std::vector<Op>& B) {
    const size_t n = A.size(), m = B.size();
    if (n == 0) return B;
    if (m == 0) return A;
    std::vector<std::vector<int>> dp(n + 1, std::vector<int>(m + 1, 0));
    for (size_t i = n; i-- > 0;)
        for (size_t j = m; j-- > 0;) {
            int best = std::max(dp[i + 1][j], dp[i][j + 1]);
            if (compatible(A[i], B[j])) best = std::max(best, dp[i + 1][j + 1] + 1);
            dp[i][j] = best;
        }
    std::vector<Op> out;
    size_t i = 0, j = 0;
    while (i < n && j < m) {
        if (compatible(A[i], B[j]) && dp[i][j] == dp[i + 1][j + 1] + 1) { out.push_back(merged(A[i], B[j])); ++i; ++j; }
        else if (dp[i + 1][j] >= dp[i][j + 1]) out.push_back(A[i++]);
        else out.push_back(B[j++]);
    }
    while (i < n) out.push_back(A[i++]);
    while (j < m) out.push_back(B[j++]);
    return out;
}

void to_launches(const m2f_plan& P, const std::vector<Op>& ops, std::vector<Launch>& out) {
    for (const Op& o : ops) {
        Launch l;
        l.kind = o.kind; l.layout = o.layout; l.src = o.src; l.group = o.group;
        memset(&l.gb, 0, sizeof(l.gb)); memset(&l.ab, 0, sizeof(l.ab)); memset(&l.lb, 0, sizeof(l.lb)); memset(&l.sb, 0, sizeof(l.sb));
        switch (o.kind) {
            case OP_GEMM:
                l.gb.count = (int)o.gp.size();
                for (size_t i = 0; i < o.gp.size(); ++i) l.gb.pr[i] = o.gp[i];
                l.gb.rng = P.rng; l.gb.drop_thresh = P.drop_thresh; l.gb.drop_scale = P.drop_scale;
                // in-launch split-K stays OFF in plans: measured 2x SLOWER on the 96-tile GEMMs (the agent-scope
                // release/acquire seam costs more than the spread saves; same verdict as the guide's M=256 block)
                l.gb.splitk_ws = nullptr; l.gb.splitk_cnt = nullptr; l.gb.splitk_max_tiles = 0;
                break;
            case OP_ATTN_FWD: case OP_ATTN_BWD:
                l.ab.count = (int)o.ap.size();
                for (size_t i = 0; i < o.ap.size(); ++i) l.ab.pr[i] = o.ap[i];
                l.ab.B = P.B; l.ab.L = P.L; l.ab.key_pad = static_cast<const uint8_t*>(P.bufs[M2F_BUF_KEYPAD]);
                l.ab.cu = P.packed ? P.cu : nullptr; l.ab.T = P.T;
                l.ab.rng = P.rng; l.ab.drop_thresh = P.drop_thresh; l.ab.drop_scale = P.drop_scale;
                m2f_attn_set_band(l.ab, P.band_past, P.band_future);
                l.ab.bias_gain16 = m2f_attn_bias_gain16(P.bias_gain);
                {   // M2F_ATTN_BF16=<mask> (read when a plan is built; AttnBatch::bf16_math): 0 keeps the fp32 slabs / contractions in bf16 mode too
                    const char* e = getenv("M2F_ATTN_BF16");
                    l.ab.bf16_math = P.prec == M2F_PREC_BF16 ? (e ? atoi(e) & 63 : 63) : 0;
                }
                break;
            case OP_LN_FWD: case OP_LN_BWD:
                l.lb.count = (int)o.lp.size();
                for (size_t i = 0; i < o.lp.size(); ++i) l.lb.pr[i] = o.lp[i];
                l.lb.T = P.T; l.lb.eps = P.cfg.ln_eps;
                l.lb.rng = P.rng; l.lb.drop_thresh = P.drop_thresh; l.lb.drop_scale = P.drop_scale;
                break;
            case OP_DROPOUT:
                l.dptr = o.dptr; l.dT = o.dT; l.dd = o.dd; l.dld = o.dld; l.dsite = o.dsite;
                // two in-place dropouts in a row over buffers of one shape (the modalities' post-projection gradients): one launch
                if (!out.empty() && out.back().kind == OP_DROPOUT && !out.back().dptr2 && out.back().group == l.group &&
                    out.back().dT == l.dT && out.back().dd == l.dd && out.back().dld == l.dld && out.back().dptr != l.dptr) {
                    out.back().dptr2 = l.dptr; out.back().dsite2 = l.dsite;
                    continue;
                }
                break;
        }
        out.push_back(l);
    }
}

// bf16 mode: which fp32 results does nobody read?  Every GEMM / attention output in the workspace is written twice - fp32 and
// its bf16 shadow - but GEMM operands, the weight-gradient table and (M2F_ATTN_BF16 bits) the attention slabs are staged from the
// shadows: the fp32 copy of a QKV projection, an attention output, an attention input gradient or an FFN hidden gradient is
// dead weight (half a gigabyte of writes per C3 step).  The readers are enumerated from the FINAL launch lists - whatever takes a
// workspace pointer as fp32 marks its extent in a map of 64-float blocks - and an output whose extent holds no mark gets
// GF_NO_F32 / AttnProblem::no_f32.  Its fp32 buffer is then filled with NaNs, once: a reader this walk does not know about
// cannot go unnoticed.  M2F_SKIP_F32=0 (read when a plan is built) keeps every fp32 store.
int mark_unread_fp32(m2f_plan& P, const float* wsf, size_t ws_floats, const std::vector<GemmProblem>& table_probs, bool poison) {
    const char* e = getenv("M2F_SKIP_F32");
    if (e && atoi(e) == 0) return 0;
    std::vector<uint8_t> read32((ws_floats + 63) / 64, 0), read16((ws_floats + 63) / 64, 0);      // fp32 readers / bf16-shadow readers
    auto span = [&](const float* p, size_t rows, size_t ld, size_t cols, size_t& lo, size_t& hi) {
        if (!p || p < wsf || p >= wsf + ws_floats || rows == 0) return false;
        lo = (size_t)(p - wsf); hi = std::min(ws_floats, lo + (rows - 1) * ld + cols);
        return hi > lo;
    };
    auto mark = [&](const float* p, size_t rows, size_t ld, size_t cols) {
        size_t lo, hi;
        if (span(p, rows, ld, cols, lo, hi)) for (size_t b = lo / 64; b <= (hi - 1) / 64; ++b) read32[b] = 1;
    };
    const uint16_t* sh0 = P.built.sh.shadow;
    auto mark16 = [&](const uint16_t* q, size_t rows, size_t ld, size_t cols) {      // q: a pointer into the activation shadow
        if (!q || !sh0 || q < sh0 || q >= sh0 + ws_floats) return;
        size_t lo, hi;
        if (span(wsf + (q - sh0), rows, ld, cols, lo, hi)) for (size_t b = lo / 64; b <= (hi - 1) / 64; ++b) read16[b] = 1;
    };
    auto unread16 = [&](const float* p, size_t rows, size_t ld, size_t cols) {
        size_t lo, hi;
        if (!span(p, rows, ld, cols, lo, hi)) return false;
        for (size_t b = lo / 64; b <= (hi - 1) / 64; ++b) if (read16[b]) return false;
        return true;
    };
    auto unread = [&](const float* p, size_t rows, size_t ld, size_t cols) {
        size_t lo, hi;
        if (!span(p, rows, ld, cols, lo, hi)) return false;
        for (size_t b = lo / 64; b <= (hi - 1) / 64; ++b) if (read32[b]) return false;
        return true;
    };
    const size_t T = (size_t)P.T;
    // buffers the caller sees (m2f_plan_buffer): always fp32-read
    auto pad8 = [](int x) { return (size_t)((x + 7) & ~7); };
    mark(static_cast<const float*>(P.bufs[M2F_BUF_TEXT]), T, pad8(P.cfg.d_text), pad8(P.cfg.d_text));
    mark(static_cast<const float*>(P.bufs[M2F_BUF_AUDIO]), T, pad8(P.cfg.d_audio), pad8(P.cfg.d_audio));
    mark(static_cast<const float*>(P.bufs[M2F_BUF_LOGITS]), T, (size_t)P.cfg.cls_out, (size_t)P.cfg.cls_out);
    mark(static_cast<const float*>(P.bufs[M2F_BUF_DLOGITS]), T, (size_t)P.cfg.cls_out, (size_t)P.cfg.cls_out);
    mark(static_cast<const float*>(P.bufs[M2F_BUF_FAM0_OUT]), T, pad8(P.cfg.d_fam), pad8(P.cfg.d_fam));
    mark(static_cast<const float*>(P.bufs[M2F_BUF_DTEXT]), T, pad8(P.cfg.d_text), pad8(P.cfg.d_text));
    mark(static_cast<const float*>(P.bufs[M2F_BUF_DAUDIO]), T, pad8(P.cfg.d_audio), pad8(P.cfg.d_audio));
    // (m2f_plan_supcon's add launch reads and rewrites the fp32 gradient of the classifier's last hidden activation; the activation itself
    // is a gate operand, marked with its launch)
    if (P.train) mark(P.crit.supcon_dh, T, pad8(P.cfg.cls_hidden), (size_t)P.cfg.cls_hidden);
    auto operand = [&](const GemmOperand& o, size_t rows_hint, bool launch16) {
        for (int sg = 0; sg < 2; ++sg)
            if (o.k[sg] > 0 && o.p[sg]) {
                const size_t rows = std::max(rows_hint, (size_t)o.k[sg]);
                if (!launch16 || !o.q[sg]) mark(o.p[sg], rows, (size_t)o.ld[sg], (size_t)o.ld[sg]);      // staged from fp32 (extent: generous)
                else mark16(o.q[sg], rows, (size_t)o.ldq[sg], (size_t)o.ldq[sg]);
            }
    };
    std::vector<std::vector<Launch>*> lists = {&P.built.fwd, &P.built.bwd, &P.built.wg_rest};
    for (std::vector<Launch>* ls : lists)
        for (Launch& l : *ls) {
            switch (l.kind) {
                case OP_GEMM: {
                    const bool launch16 = m2f_gemm_stages_bf16(l.gb, l.layout);      // (one operand without a shadow sends the whole launch to fp32 staging)
                    for (int i = 0; i < l.gb.count; ++i) {
                        const GemmProblem& g = l.gb.pr[i];
                        const size_t big = (size_t)std::max(std::max(g.M, g.N), (int)T);
                        operand(g.a, big, launch16); operand(g.b, big, launch16);
                        mark(g.res, (size_t)g.M, (size_t)g.ldres, (size_t)g.N);
                        mark(g.gate, (size_t)g.M, (size_t)g.ldgate, (size_t)g.N);
                        if (g.flags & GF_ACCUM) mark(g.c, (size_t)g.M, (size_t)g.ldc, (size_t)g.N);
                    }
                    break;
                }
                case OP_ATTN_FWD: case OP_ATTN_BWD:
                    for (int i = 0; i < l.ab.count; ++i) {
                        const AttnProblem& a = l.ab.pr[i];
                        const size_t w = (size_t)a.H * a.hd;
                        // (the streaming kernel reads the fp32 rows and rounds them itself)
                        const int bits = P.streaming ? 0 : m2f_attn_shadow_only_bits(l.ab, i, l.kind == OP_ATTN_BWD);
                        auto rd = [&](const float* p, int ld, int bit) {
                            if (!p) return;
                            if (bits & bit) mark16(sh0 + (p - wsf), T, (size_t)ld, w); else mark(p, T, (size_t)ld, w);
                        };
                        rd(a.q, a.ldq, 2); rd(a.k, a.ldk, 4); rd(a.v, a.ldv, 8);
                        if (l.kind == OP_ATTN_BWD) { rd(a.dout, a.lddo, 16); rd(a.out, a.ldo, 32); }
                    }
                    break;
                case OP_LN_FWD: case OP_LN_BWD:
                    for (int i = 0; i < l.lb.count; ++i) {
                        const LnProblem& q = l.lb.pr[i];
                        const size_t ld = (size_t)(q.ld ? q.ld : q.d);
                        mark(q.x, T, ld, (size_t)q.d);
                        mark(q.res, T, ld, (size_t)q.d);
                        if (l.kind == OP_LN_BWD) { mark(q.dy, T, ld, (size_t)q.d); mark(q.extra, T, ld, (size_t)q.d); }
                    }
                    break;
                case OP_DROPOUT: mark(l.dptr, (size_t)l.dT, (size_t)l.dld, (size_t)l.dd); mark(l.dptr2, (size_t)l.dT, (size_t)l.dld, (size_t)l.dd); break;
                default: break;
            }
        }
    for (const CastBatch& cb : P.built.wg_casts)
        for (int i = 0; i < cb.count; ++i) mark(cb.it[i].src, (size_t)cb.it[i].rows, (size_t)cb.it[i].lds, (size_t)cb.it[i].cols);
    // (the weight-gradient table stages bf16 shadows only - what it cannot take went to wg_rest / wg_casts above; the criterion
    // reads the logits, marked with the caller-visible buffers)
    for (const GemmProblem& g : table_probs) {
        mark16(g.a.q[0], T, (size_t)g.a.ldq[0], (size_t)g.a.ldq[0]);
        mark16(g.b.q[0], T, (size_t)g.b.ldq[0], (size_t)g.b.ldq[0]);
    }
    int n = 0;
    auto poison_buf = [&](float* p, size_t rows, size_t ld, size_t cols) {
        size_t lo, hi;
        if (!poison || !span(p, rows, ld, cols, lo, hi)) return 0;
        return hipMemset(p, 0xFF, (hi - lo) * sizeof(float)) == hipSuccess ? 0 : 1;
    };
    auto poison16 = [&](const float* p, size_t rows, size_t ld, size_t cols) {       // ... and a shadow that is no longer written
        size_t lo, hi;
        if (!poison || !sh0 || !span(p, rows, ld, cols, lo, hi)) return 0;
        return hipMemset(const_cast<uint16_t*>(sh0) + lo, 0xFF, (hi - lo) * sizeof(uint16_t)) == hipSuccess ? 0 : 1;
    };
    for (std::vector<Launch>* ls : {&P.built.fwd, &P.built.bwd})
        for (Launch& l : *ls) {
            if (l.kind == OP_GEMM) {
                for (int i = 0; i < l.gb.count; ++i) {
                    GemmProblem& g = l.gb.pr[i];
                    if (unread16(g.c, (size_t)g.M, (size_t)g.ldc, (size_t)g.N)) {      // nobody stages C's shadow
                        g.flags |= GF_NO_BF16; ++n;
                        if (poison16(g.c, (size_t)g.M, (size_t)g.ldc, (size_t)g.N)) return fail("mark_unread_fp32: hipMemset");
                    }
                    if ((g.flags & (GF_ACCUM | GF_NO_BF16)) || g.c8 || !unread(g.c, (size_t)g.M, (size_t)g.ldc, (size_t)g.N)) continue;
                    g.flags |= GF_NO_F32; ++n;
                    if (poison_buf(g.c, (size_t)g.M, (size_t)g.ldc, (size_t)g.N)) return fail("mark_unread_fp32: hipMemset");
                }
            } else if (l.kind == OP_LN_BWD) {
                for (int i = 0; i < l.lb.count; ++i) {
                    LnProblem& q = l.lb.pr[i];
                    const size_t ld = (size_t)(q.ld ? q.ld : q.d);
                    if (q.dx_masked && unread(q.dx_masked, T, ld, (size_t)q.d)) {
                        q.skip |= 1u; ++n;
                        if (poison_buf(q.dx_masked, T, ld, (size_t)q.d)) return fail("mark_unread_fp32: hipMemset");
                    }
                    if (unread16(q.dx, T, ld, (size_t)q.d)) {
                        q.skip |= 2u; ++n;
                        if (poison16(q.dx, T, ld, (size_t)q.d)) return fail("mark_unread_fp32: hipMemset");
                    }
                }
            } else if (l.kind == OP_ATTN_FWD && !P.streaming) {
                for (int i = 0; i < l.ab.count; ++i) {
                    AttnProblem& a = l.ab.pr[i];
                    const size_t w = (size_t)a.H * a.hd;
                    if (!unread(a.out, T, (size_t)a.ldo, w)) continue;
                    a.no_f32 = 1; ++n;
                    if (poison_buf(a.out, T, (size_t)a.ldo, w)) return fail("mark_unread_fp32: hipMemset");
                }
            } else if (l.kind == OP_ATTN_BWD) {
                for (int i = 0; i < l.ab.count; ++i) {
                    AttnProblem& a = l.ab.pr[i];
                    const size_t w = (size_t)a.H * a.hd;
                    if (!unread(a.dq, T, (size_t)a.lddq, w) || !unread(a.dk, T, (size_t)a.lddk, w) || !unread(a.dv, T, (size_t)a.lddv, w)) continue;
                    a.no_f32 = 1; ++n;
                    if (poison_buf(a.dq, T, (size_t)a.lddq, w) || poison_buf(a.dk, T, (size_t)a.lddk, w) || poison_buf(a.dv, T, (size_t)a.lddv, w))
                        return fail("mark_unread_fp32: hipMemset");
                }
            }
        }
    P.built.n_no_f32 = n;
    return 0;
}

// The backward launch lists of a train plan: the head chain (classifier + fusion stack), then the merged branches; the deferred
// weight gradients as grouped launches in dependency order; the LayerNorm parameter reduces.
void build_backward(m2f_plan& P, Builder& bld) {
    for (size_t i = 0; i < bld.chain_b.size(); ++i) bld.chain_b[i].src.push_back({2, (int)i});
    for (int b = 0; b < 2; ++b)
        for (size_t i = 0; i < bld.br_b[b].size(); ++i) bld.br_b[b][i].src.push_back({b, (int)i});
    to_launches(P, bld.chain_b, P.built.bwd);
    P.built.bwd_head = P.built.bwd.size();
    to_launches(P, merge_chains(bld.br_b[0], bld.br_b[1]), P.built.bwd);
    // input gradients (m2f_plan_backward_outputs): behind both branch chains, both modalities in one grouped launch.  Nothing reads
    // them, so the launches before them - and the weight gradients those feed - are the default backward's, launch for launch.
    to_launches(P, merge_chains(bld.in_b[0], bld.in_b[1]), P.built.bwd);
    // where did (chain, index) end up in the final launch order?
    auto final_index = [&](std::pair<int, int> tag) {
        if (tag.second < 0) return tag.first == 2 ? -1 : (int)bld.chain_b.size() - 1;   // before the branch: after the head
        for (size_t i = 0; i < P.built.bwd.size(); ++i)
            for (const auto& sidx : P.built.bwd[i].src)
                if (sidx == tag) return (int)i;
        return (int)P.built.bwd.size() - 1;
    };
    // deferred weight gradients: chip-filling grouped launches, in dependency order
    std::vector<std::pair<int, size_t>> order;
    for (size_t i = 0; i < bld.wgrads.size(); ++i) order.push_back({final_index(bld.wdeps[i]), i});
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    // groups of up to 8 problems; a problem that cannot be staged from bf16 shadows (leading dimension not a
    // multiple of 8: the [T, n_classes] criterion gradient) gets a launch of its own instead of dragging seven
    // others onto the fp32-source path
    std::vector<Op> wops;
    auto shadowable = [](const GemmProblem& g) { return !(g.a.ld[0] & 7) && !(g.b.ld[0] & 7); };
    size_t i = 0;
    while (i < order.size()) {
        Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_TN;
        const bool kind0 = shadowable(bld.wgrads[order[i].second]);
        while (i < order.size() && o.gp.size() < M2F_GEMM_MAX_PROBLEMS && shadowable(bld.wgrads[order[i].second]) == kind0) {
            o.gp.push_back(bld.wgrads[order[i].second]);
            ++i;
        }
        wops.push_back(o);
    }
    to_launches(P, wops, P.built.wg);
    for (size_t i = 0; i < bld.lnitems.size(); i += M2F_LNRED_MAX_ITEMS) {
        LnReduceBatch rb;
        memset(&rb, 0, sizeof(rb));
        for (size_t j = i; j < std::min(bld.lnitems.size(), i + M2F_LNRED_MAX_ITEMS); ++j) rb.it[rb.count++] = bld.lnitems[j];
        P.built.lnred.push_back(rb);
    }
}

// Per-workgroup tile lists of the weight-gradient table (m2f_gemm_table_walk) and their place in the workspace
struct TableTiles { std::vector<uint32_t> rec; std::vector<int> begin; int n_wg = 0; uint32_t* d_rec = nullptr; int* d_begin = nullptr; };

// The tile lists over the problems `sub` (null: all of them): walked for 256 workgroups, and again for as many workgroups as
// there are tiles when there are fewer.  False when a walk fails.
bool walk_table(const std::vector<GemmProblem>& probs, int walk, int tile_m, int tile_n, const std::vector<int>* sub, TableTiles& t) {
    if (m2f_gemm_table_walk(probs, walk, 256, tile_m, tile_n, t.rec, t.begin, sub) <= 0) return false;
    t.n_wg = std::min((int)t.rec.size(), 256);
    return t.n_wg == 256 || m2f_gemm_table_walk(probs, walk, t.n_wg, tile_m, tile_n, t.rec, t.begin, sub) > 0;
}

// The weight-gradient table (bf16 mode): its problems `tprobs` on the activation shadows (narrow operands: padded copies, wg_casts;
// the rest: wg_rest), its tile lists for the step and each part of the split step, their arena space (the same in the sizing pass),
// and in the real pass of a bf16 plan the upload and wg_tab / wg_tab_part.  Returns whether the table can run.
bool build_wgrad_table(m2f_plan& P, Builder& bld, char* ws_base, uint16_t* shadow, size_t ws_floats, std::vector<GemmProblem>& tprobs) {
    const int T = P.T;
    std::vector<int> tprob_head, tprob_rest;   // indices into tprobs by backward part (m2f_step_part)
    size_t rest_head = 0;
    // M2F_WGRAD_TABLE=0 (read when a plan is built) keeps the grouped row-contiguous launches in bf16 mode too: the parity
    // tests compare the two weight-gradient paths against each other
    const char* wg_env = getenv("M2F_WGRAD_TABLE");
    bool table_ok = P.train && !bld.wgrads.empty() && !(wg_env && wg_env[0] == '0');
    // The launch reads the ROW-MAJOR bf16 shadows the chain already maintains and sums the bias gradients itself.  Its form,
    // M2F_TABLE_TILE (read when a plan is built): 132 (default; any value but 131) = 256 x 256 tiles on the eight-phase
    // schedule (gemm_p8.h); 131 = the ring form (gemm_ring.h) with 256 (M) x 128 (N) tiles.  The launch is bound by the bytes
    // its 256 workgroups pull through the L2s together (26.0 M L1->L2 requests per launch at C3 with 128x128 tiles, 19.5 M
    // with 256x128; 361 -> 290 us, profiles/r03_*).  DESIGN.md section 3 has the forms measured before these.
    const char* tt_env = getenv("M2F_TABLE_TILE");
    bool table_p8 = !(tt_env && atoi(tt_env) == 131);
    if (table_ok) {
        // operands = shadows of the fp32 activations (same element index); every one of them is also the A operand of a
        // forward-form chain launch, so its shadow is current when the backward chain has run
        const float* wsf = reinterpret_cast<const float*>(ws_base);
        auto shadow_ptr = [&](const float* ptr) -> const uint16_t* {
            if (!ws_base) return reinterpret_cast<const uint16_t*>(16);           // sizing pass: any non-null, aligned value
            const ptrdiff_t i = ptr - wsf;
            return (i >= 0 && (size_t)i < ws_floats) ? shadow + i : nullptr;
        };
        std::vector<Op> rest_ops;
        CastBatch wg_cast;
        memset(&wg_cast, 0, sizeof(wg_cast));
        for (size_t gi = 0; gi < bld.wgrads.size(); ++gi) {
            const GemmProblem& g = bld.wgrads[gi];
            const bool head = bld.wdeps[gi].first == 2;        // both operands exist once the classifier / fusion backward chain has run
            const uint16_t* qa = shadow_ptr(g.a.p[0]);
            const uint16_t* qb = shadow_ptr(g.b.p[0]);
            if (g.a.k[1] != 0 || g.b.k[1] != 0) { table_ok = false; break; }
            int lda = g.a.ld[0];
            const bool b_ok = qb && !(g.b.ld[0] & 7) && !(reinterpret_cast<uintptr_t>(qb) & 15) && (size_t)T * g.b.ld[0] * 2 < 0x80000000ull;
            if (b_ok && g.M <= 8 && !(g.flags & GF_RELU_A) && wg_cast.count < M2F_CAST_MAX_ITEMS) {
                // a narrow dY without a 16-byte-stageable shadow (the [T, n_classes] criterion gradient): a bf16 copy with
                // 8-column rows, made by a cast launch in front of the table launch (the pad column is zeroed once, here)
                uint16_t* pad = bld.ar.alloc<uint16_t>((size_t)T * 8 + 256);      // + one 512-byte fragment row (256-row tiles) past the end
                if (ws_base && hipMemset(pad, 0, ((size_t)T * 8 + 256) * sizeof(uint16_t)) != hipSuccess) { table_ok = false; break; }
                CastItem& ci = wg_cast.it[wg_cast.count++];
                ci.src = g.a.p[0]; ci.dst = pad; ci.rows = T; ci.cols = g.M; ci.lds = g.a.ld[0]; ci.ldd = 8; ci.dst_t = nullptr; ci.ldd_t = 0;
                qa = pad; lda = 8;
            }
            if (!qa || !b_ok || (lda & 7) || (reinterpret_cast<uintptr_t>(qa) & 15) || (size_t)T * lda * 2 >= 0x80000000ull) {
                // no 16-byte-stageable shadow (the [T, n_classes] criterion gradient): a grouped launch of its own
                Op o; o.kind = OP_GEMM; o.layout = M2F_LAYOUT_TN;
                o.gp.push_back(g);
                if (head) { rest_ops.insert(rest_ops.begin() + (ptrdiff_t)rest_head, o); ++rest_head; } else rest_ops.push_back(o);
                continue;
            }
            GemmProblem q;
            memset(&q, 0, sizeof(q));
            q.a.q[0] = qa; q.a.ldq[0] = lda; q.a.k[0] = T;
            q.b.q[0] = qb; q.b.ldq[0] = g.b.ld[0]; q.b.k[0] = T;
            q.M = g.M; q.N = g.N; q.c = g.c; q.ldc = g.ldc; q.gate_scale = 1.f;
            q.flags = g.flags & (uint32_t)(GF_RELU_A | GF_RELU_B);
            q.bias_grad = g.bias_grad;
            (head ? tprob_head : tprob_rest).push_back((int)tprobs.size());
            tprobs.push_back(q);
            P.built.wg_flops += 2.0 * g.M * g.N * (double)T;
        }
        if (table_ok) { to_launches(P, rest_ops, P.built.wg_rest); P.built.wg_rest_head = rest_head; }
        if (table_ok && wg_cast.count) P.built.wg_casts.push_back(wg_cast);
    }
    // the table kernels stage the operands as they are and store plain results: no epilogue terms, one segment per operand
    for (const GemmProblem& q : tprobs)
        if ((q.flags & (GF_RELU_OUT | GF_ACCUM | GF_GELU_OUT)) || q.bias || q.res || q.gate || q.drop_site || q.c8 || q.a.k[1] || q.b.k[1]) table_ok = false;
    if (table_p8 && table_ok && !m2f_gemm_p8_table_ok(tprobs)) table_p8 = false;      // (a problem with ReLU on its A operand: the eight-phase form has no loop copy for it)
    const int walk_m = 256, walk_n = table_p8 ? 256 : 128;
    // M2F_TABLE_WALK=0 (read when a plan is built) keeps the order of the tile list; default 1 = every XCD walks its own problems
    // in 8 x 4 super-tiles
    const char* walk_env = getenv("M2F_TABLE_WALK");
    const int walk = walk_env ? atoi(walk_env) : 1;
    TableTiles tl[3];                          // the whole table; the problems of part 0 and of part 1 of the split step
    if (table_ok) table_ok = walk_table(tprobs, walk, walk_m, walk_n, nullptr, tl[0]);
    bool split = table_ok && P.built.bwd_head > 0 && P.built.bwd_head < P.built.bwd.size() && !tprob_head.empty() && !tprob_rest.empty();
    for (int part = 0; part < 2 && split; ++part)
        split = walk_table(tprobs, walk, walk_m, walk_n, part == 0 ? &tprob_head : &tprob_rest, tl[1 + part]);
    const int n_lists = !table_ok ? 0 : split ? 3 : 1;
    GemmProblem* d_table = table_ok ? bld.ar.alloc<GemmProblem>(tprobs.size()) : nullptr;
    for (int i = 0; i < n_lists; ++i) {        // (same allocations in the sizing pass: neither `table_ok` nor `split` depends on pointers)
        tl[i].d_rec = bld.ar.alloc<uint32_t>(tl[i].rec.size());
        tl[i].d_begin = bld.ar.alloc<int>(tl[i].begin.size());
    }
    if (!table_ok || P.prec != M2F_PREC_BF16 || ws_base == nullptr) return table_ok;
    bool ok = hipMemcpy(d_table, tprobs.data(), tprobs.size() * sizeof(GemmProblem), hipMemcpyHostToDevice) == hipSuccess;
    P.built.tprobs_host = tprobs;
    for (int i = 0; i < n_lists; ++i) {
        ok = ok && hipMemcpy(tl[i].d_rec, tl[i].rec.data(), tl[i].rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(tl[i].d_begin, tl[i].begin.data(), tl[i].begin.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) return table_ok;
    auto set_tiles = [](GemmBatch& b, const TableTiles& t) {
        b.tile_rec = t.d_rec; b.wg_begin = t.d_begin; b.wg_count = t.n_wg; b.total_tiles = (int)t.rec.size();
        b.p8_max_tiles = 0;
        for (size_t w = 0; w + 1 < t.begin.size(); ++w) b.p8_max_tiles = std::max(b.p8_max_tiles, t.begin[w + 1] - t.begin[w]);
    };
    P.built.wg_table = true;
    memset(&P.built.wg_tab, 0, sizeof(P.built.wg_tab));
    P.built.wg_tab.table = d_table; P.built.wg_tab.table_p8 = table_p8;
    P.built.wg_tab.rng = P.rng; P.built.wg_tab.drop_thresh = P.drop_thresh; P.built.wg_tab.drop_scale = P.drop_scale;
    set_tiles(P.built.wg_tab, tl[0]);
    for (int part = 0; part < 2 && split; ++part) { P.built.wg_tab_part[part] = P.built.wg_tab; set_tiles(P.built.wg_tab_part[part], tl[1 + part]); }
    // the fusion stack's (else the classifier's) first parameter: everything from there on is complete after part 0
    P.built.split_ok = split;
    P.built.split_offset = (int64_t)(P.cfg.fam_enabled && !P.pm.fam.empty() ? P.pm.fam[0].in_w : P.pm.cls[0].w);
    return table_ok;
}

// bf16 mode, real pass: every launch's shadow map, the chain GEMMs' bf16 operands (activations: same element index; 2-D parameters:
// their padded W and W^T shadows), and the casts that refresh the parameter and input shadows at the start of a forward.
void map_shadows(m2f_plan& P, const float* wsf, uint16_t* shadow, size_t ws_floats, uint16_t* wshadow) {
    const m2f_config& c = P.cfg;
    const int T = P.T;
    P.built.sh = {wsf, shadow, ws_floats};
    P.built.wshadow = wshadow;
    P.built.wg_tab.sh = P.built.sh;
    P.built.wg_tab_part[0].sh = P.built.sh; P.built.wg_tab_part[1].sh = P.built.sh;
    auto map_q = [&](GemmOperand& o) {
        for (int sgm = 0; sgm < 2; ++sgm) {
            o.q[sgm] = nullptr; o.ldq[sgm] = 0; o.qt[sgm] = nullptr; o.ldqt[sgm] = 0;
            const float* p = o.p[sgm];
            if (o.k[sgm] == 0 || !p) continue;
            const float* dl = static_cast<const float*>(P.bufs[M2F_BUF_DLOGITS]);
            if (p >= dl && p < dl + (size_t)T * c.cls_out) continue;          // written by the criterion kernel: no shadow
            if (p >= wsf && p < wsf + ws_floats) { o.q[sgm] = shadow + (p - wsf); o.ldq[sgm] = o.ld[sgm]; continue; }
            if (p >= P.params && p < P.params + P.pm.total) {
                const size_t idx = (size_t)(p - P.params);
                for (const ParamMap::Mat& m : P.pm.mats) {
                    if (idx >= m.off && idx < m.off + (size_t)m.rows * m.cols && o.ld[sgm] == m.cols) {
                        const size_t r = (idx - m.off) / m.cols, cc = (idx - m.off) % m.cols;
                        o.ldq[sgm] = (m.cols + 7) & ~7;
                        o.q[sgm] = wshadow + m.soff + r * o.ldq[sgm] + cc;
                        o.ldqt[sgm] = (m.rows + 7) & ~7;                       // W^T shadow: [cols][pad8(rows)]
                        o.qt[sgm] = wshadow + m.soff_t + cc * o.ldqt[sgm] + r;
                        break;
                    }
                }
            }
        }
    };
    for (std::vector<Launch>* ls : {&P.built.fwd, &P.built.bwd, &P.built.wg})
        for (Launch& l : *ls) {
            l.gb.sh = P.built.sh; l.ab.sh = P.built.sh; l.lb.sh = P.built.sh; l.sb.sh = P.built.sh;
            if (l.kind == OP_GEMM)
                for (int i = 0; i < l.gb.count; ++i) { map_q(l.gb.pr[i].a); map_q(l.gb.pr[i].b); }
        }
    // casts at the start of a forward: every 2-D parameter into its padded shadow, then the two input buffers
    CastBatch cb;
    memset(&cb, 0, sizeof(cb));
    std::vector<CastBatch>* dst = &P.built.param_casts;
    auto flush = [&]() { if (cb.count) { dst->push_back(cb); memset(&cb, 0, sizeof(cb)); } };
    for (const ParamMap::Mat& m : P.pm.mats) {
        cb.it[cb.count++] = {P.params + m.off, wshadow + m.soff, m.rows, m.cols, m.cols, (m.cols + 7) & ~7,
                             wshadow + m.soff_t, (m.rows + 7) & ~7};
        if (cb.count == M2F_CAST_MAX_ITEMS) flush();
    }
    flush();
    dst = &P.built.input_casts;
    if (c.text_enabled) {
        const int dp = Builder::pad8(c.d_text);
        float* x = static_cast<float*>(P.bufs[M2F_BUF_TEXT]);
        cb.it[cb.count++] = {x, shadow + (x - wsf), T, c.d_text, dp, dp, nullptr, 0};
    }
    if (c.audio_enabled) {
        const int dp = Builder::pad8(c.d_audio);
        float* x = static_cast<float*>(P.bufs[M2F_BUF_AUDIO]);
        cb.it[cb.count++] = {x, shadow + (x - wsf), T, c.d_audio, dp, dp, nullptr, 0};
    }
    flush();
}

// Stream plans: the per-slot counters and every attention site's K / V caches, behind everything the activation shadows mirror (the
// caches are the bulk of a stream plan's workspace and have no shadow); each OP_ATTN_FWD launch gets its streaming form.
void build_stream_sites(m2f_plan& P, Builder& bld) {
    const int S = P.B, bf16 = P.prec == M2F_PREC_BF16;
    P.s_len = bld.ar.alloc<int>((size_t)S);
    P.s_active = bld.ar.alloc<uint8_t>((size_t)S);
    P.bufs[M2F_BUF_STREAM_LEN] = P.s_len;
    P.bufs[M2F_BUF_STREAM_ACTIVE] = P.s_active;
    size_t cache_bytes = 0;
    for (Launch& l : P.built.fwd) {
        if (l.kind != OP_ATTN_FWD) continue;
        AttnStreamBatch& sb = l.sb;
        memset(&sb, 0, sizeof(sb));
        sb.count = l.ab.count; sb.S = S; sb.C = P.s_cap; sb.ring = P.s_ring; sb.bf16 = bf16;
        sb.len = P.s_len; sb.active = P.s_active; sb.bias_gain = P.bias_gain;
        for (int i = 0; i < l.ab.count; ++i) {
            const AttnProblem& a = l.ab.pr[i];
            AttnStreamProblem& q = sb.pr[i];
            q.q = a.q; q.k = a.k; q.v = a.v; q.ldq = a.ldq; q.ldk = a.ldk; q.ldv = a.ldv; q.out = a.out; q.ldo = a.ldo; q.H = a.H; q.hd = a.hd;
            const size_t n = P.s_pages ? m2f_attn_stream_pool_elems(P.s_pages, a.H, a.hd, P.s_pg.R, bf16)
                                       : m2f_attn_stream_cache_elems(S, a.H, a.hd, P.s_cap, bf16);
            if (bf16) { q.kcache = bld.ar.alloc<uint16_t>(n); q.vcache = bld.ar.alloc<uint16_t>(n); }
            else { q.kcache = bld.ar.alloc<float>(n); q.vcache = bld.ar.alloc<float>(n); }
            cache_bytes += 2 * n * (bf16 ? sizeof(uint16_t) : sizeof(float));
        }
    }
    P.s_cache_bytes = (int64_t)cache_bytes;          // (the arena's alignment gaps between caches are not counted)
    if (P.s_pages) {                                 // the page table, behind the pools
        int* table = bld.ar.alloc<int>((size_t)S * P.s_pg.tw);
        P.s_pg.table = table;
        P.bufs[M2F_BUF_STREAM_TABLE] = table;
    }
}

// Chunk plans: the same sites in the same launches as the parent's (the launch lists depend on the configuration alone), each taking
// the parent's caches; the counters are the parent's, the per-slot chunk lengths are the plan's own.
int build_chunk_sites(m2f_plan& P, Builder& bld) {
    const m2f_plan& par = *P.s_parent;
    P.s_len = par.s_len;
    P.s_new = bld.ar.alloc<int>((size_t)P.B);
    P.bufs[M2F_BUF_STREAM_LEN] = P.s_len;
    P.bufs[M2F_BUF_STREAM_NEW] = P.s_new;
    P.bufs[M2F_BUF_STREAM_TABLE] = par.bufs[M2F_BUF_STREAM_TABLE];
    if (P.built.fwd.size() != par.built.fwd.size()) return fail("chunk plan: its launch list differs from the stream plan's");
    for (size_t li = 0; li < P.built.fwd.size(); ++li) {
        Launch& l = P.built.fwd[li];
        const Launch& pl = par.built.fwd[li];
        if (l.kind != pl.kind) return fail("chunk plan: its launch list differs from the stream plan's");
        if (l.kind != OP_ATTN_FWD) continue;
        if (l.ab.count != pl.sb.count) return fail("chunk plan: an attention launch differs from the stream plan's");
        AttnStreamBatch& sb = l.sb;
        memset(&sb, 0, sizeof(sb));
        sb.count = l.ab.count; sb.S = P.B; sb.C = P.s_cap; sb.ring = P.s_ring; sb.bf16 = P.prec == M2F_PREC_BF16;
        sb.len = P.s_len; sb.active = nullptr; sb.bias_gain = P.bias_gain;
        for (int i = 0; i < l.ab.count; ++i) {
            const AttnProblem& a = l.ab.pr[i];
            const AttnStreamProblem& pq = pl.sb.pr[i];
            if (a.H != pq.H || a.hd != pq.hd) return fail("chunk plan: an attention site differs from the stream plan's");
            AttnStreamProblem& q = sb.pr[i];
            q.q = a.q; q.k = a.k; q.v = a.v; q.ldq = a.ldq; q.ldk = a.ldk; q.ldv = a.ldv; q.out = a.out; q.ldo = a.ldo; q.H = a.H; q.hd = a.hd;
            q.kcache = pq.kcache; q.vcache = pq.vcache;
        }
    }
    return 0;
}

}  // namespace

namespace m2f {

void apply_speakers(m2f_plan& P) {
    const bool on = (P.spk_same | P.spk_other) != 0;
    const uint8_t* ids = on ? static_cast<const uint8_t*>(P.bufs[M2F_BUF_SPEAKERS]) : nullptr;
    for (Launch& l : P.built.fwd) {                      // (forward only: the backward kernels read the saved probabilities)
        if (l.kind != OP_ATTN_FWD) continue;
        l.ab.speaker = ids; l.ab.spk_same = (uint8_t)(on ? P.spk_same : 0); l.ab.spk_other = (uint8_t)(on ? P.spk_other : 0);
        if (P.streaming) {
            l.sb.spk_cache = on ? P.s_spk : nullptr; l.sb.spk_new = ids;
            l.sb.spk_same = l.ab.spk_same; l.sb.spk_other = l.ab.spk_other;
        }
    }
}

int build_plan(m2f_plan& P, char* ws_base) {
    const m2f_config& c = P.cfg;
    Builder bld(P);
    bld.ar.base = ws_base;
    const int T = P.T;
    // host-visible input staging: rows padded to a multiple of 8 floats (like every activation buffer)
    P.bufs[M2F_BUF_TEXT] = bld.ar.f((size_t)T * Builder::pad8(std::max(c.d_text, 1)));
    P.bufs[M2F_BUF_AUDIO] = bld.ar.f((size_t)T * Builder::pad8(std::max(c.d_audio, 1)));
    P.bufs[M2F_BUF_KEYPAD] = bld.ar.alloc<uint8_t>((size_t)T);
    P.cu = bld.ar.alloc<int>((size_t)P.B + 1);
    P.bufs[M2F_BUF_CU_SEQLENS] = P.cu;
    P.bufs[M2F_BUF_LABELS] = bld.ar.alloc<int64_t>((size_t)T);
    P.bufs[M2F_BUF_CLASSW] = bld.ar.f(16);
    // input gradients (m2f_plan_backward_outputs): allocated in every train plan, so that the setting does not move any buffer
    P.bufs[M2F_BUF_DTEXT] = (P.train && c.text_enabled) ? bld.ar.f((size_t)T * Builder::pad8(c.d_text)) : nullptr;
    P.bufs[M2F_BUF_DAUDIO] = (P.train && c.audio_enabled) ? bld.ar.f((size_t)T * Builder::pad8(c.d_audio)) : nullptr;
    if (c.audio_enabled)
        bld.build_modality(0, P.pm.audio, c.d_audio, c.nhead_audio, c.nlayers_audio, c.ntrans_audio,
                           static_cast<const float*>(P.bufs[M2F_BUF_AUDIO]));
    if (c.text_enabled)
        bld.build_modality(1, P.pm.text, c.d_text, c.nhead_text, c.nlayers_text, c.ntrans_text,
                           static_cast<const float*>(P.bufs[M2F_BUF_TEXT]));
    bld.build_head();
    for (int bi = 0; bi < 2; ++bi)
        for (size_t e = 0; e < bld.mod[bi].L.size(); ++e)
            for (size_t l = 0; l < bld.mod[bi].L[e].size(); ++l)
                P.built.attn_sites.push_back({bi, (int)e, (int)l, bld.mod[bi].H, bld.mod[bi].d / bld.mod[bi].H, bld.mod[bi].L[e][l].probs});
    for (size_t i = 0; i < bld.fam.size(); ++i)
        P.built.attn_sites.push_back({2, (int)i, 0, c.nhead_fam, c.d_fam / c.nhead_fam, bld.fam[i].probs});
    // forward: merged branches, then fusion + classifier
    to_launches(P, merge_chains(bld.br_f[0], bld.br_f[1]), P.built.fwd);
    to_launches(P, bld.chain_f, P.built.fwd);
    if (P.train) build_backward(P, bld);
    // (behind every buffer a forward or backward launch points to: none of them moves)
    P.eval_partial = bld.ar.alloc<int>((size_t)M2F_EVAL_MAX_BLOCKS * M2F_EVAL_MAX_C * M2F_EVAL_MAX_C);
    // ---- bf16 shadows: activation shadow = one bf16 per fp32 workspace element; parameter shadow = padded matrices
    bld.ar.off = (bld.ar.off + 255) / 256 * 256;
    const size_t ws_floats = bld.ar.off / 4;
    uint16_t* shadow = bld.ar.alloc<uint16_t>(ws_floats);
    uint16_t* wshadow = P.ext_wshadow ? P.ext_wshadow : bld.ar.alloc<uint16_t>(P.pm.shadow_elems + 64);
    std::vector<GemmProblem> tprobs;
    const bool table_ok = build_wgrad_table(P, bld, ws_base, shadow, ws_floats, tprobs);
    if (P.s_parent) { if (int r = build_chunk_sites(P, bld)) return r; }
    else if (P.streaming) build_stream_sites(P, bld);
    // inputs of the distillation criterion (m2f_plan_distill), train plans only: at the very end of the workspace, behind the shadows and
    // the tables - every other buffer of the plan sits where it sat without them
    P.bufs[M2F_BUF_TEACHER] = P.train ? bld.ar.f((size_t)T * c.cls_out) : nullptr;
    P.bufs[M2F_BUF_DISTILL] = P.train ? bld.ar.f(2) : nullptr;
    // the speaker ids of the token rows (m2f_plan_attention_speakers), one byte each: behind everything again, in every plan
    P.bufs[M2F_BUF_SPEAKERS] = bld.ar.alloc<uint8_t>(((size_t)T + 15) & ~(size_t)15);
    P.bufs[M2F_BUF_STREAM_SPEAKERS] = P.s_spk;
    apply_speakers(P);
    // gamma of the focal criterion (m2f_plan_focal), one float, train and eval plans: behind everything once more, so nothing moves
    P.bufs[M2F_BUF_FOCAL] = bld.ar.f(1);
    // workspace of the CRF criterion (m2f_plan_crf), train and eval plans whose classifier has 2 .. 16 classes: behind everything again
    if (!P.streaming && !P.s_parent && c.cls_out >= 2 && c.cls_out <= 16) {
        P.crit.crf_ws = bld.ar.f((size_t)T * (2 * c.cls_out + 2) + (size_t)P.B * (c.cls_out * c.cls_out + 2 * c.cls_out));
        P.crit.crf_pred = bld.ar.alloc<int32_t>((size_t)T);
        P.crit.crf_score = bld.ar.f((size_t)P.B);
    }
    // inputs of the R-Drop criterion (m2f_plan_rdrop), train plans only: the twin map, alpha, and the per-row KL terms - behind everything again
    P.bufs[M2F_BUF_PARTNER] = P.train ? bld.ar.alloc<int32_t>((size_t)T) : nullptr;
    P.bufs[M2F_BUF_RDROP] = P.train ? bld.ar.f(1) : nullptr;
    P.crit.rdrop_kl = P.train ? bld.ar.f((size_t)T) : nullptr;
    // the supervised contrastive criterion (m2f_plan_supcon), train plans only: (lambda, tau), the kernels' workspace, the row terms, the
    // gradient w.r.t. the stored activation and the step's scale - behind everything again
    P.bufs[M2F_BUF_SUPCON] = P.train ? bld.ar.f(2) : nullptr;
    P.crit.supcon_ws = P.train ? bld.ar.f(m2f_supcon_ws_floats(T, c.cls_hidden)) : nullptr;
    P.crit.supcon_rows = P.train ? bld.ar.f((size_t)T * 4) : nullptr;
    P.crit.supcon_dfeat = P.train ? bld.ar.f((size_t)T * Builder::pad8(c.cls_hidden)) : nullptr;
    P.crit.supcon_scale = P.train ? bld.ar.f(1) : nullptr;
    // the auxiliary label head (m2f_plan_aux_head), train plans only: (lambda, eps_a), the second labels, the head's logits and the kernels'
    // workspace sized for 16 classes - behind everything again, whether or not the switch is on
    P.bufs[M2F_BUF_AUX] = P.train ? bld.ar.f(2) : nullptr;
    P.bufs[M2F_BUF_AUX_LABELS] = P.train ? bld.ar.alloc<int64_t>((size_t)T) : nullptr;
    P.bufs[M2F_BUF_AUX_LOGITS] = P.train ? bld.ar.f((size_t)T * 16) : nullptr;
    P.crit.aux_ws = P.train && c.cls_hidden <= 1024 ? bld.ar.f(m2f_aux_head_ws_floats(T, c.cls_hidden, 16)) : nullptr;
    P.crit.aux_scale = P.train ? bld.ar.f(1) : nullptr;
    P.built.ws_used = bld.ar.off;
    if (P.prec == M2F_PREC_BF16 && ws_base != nullptr) {
        const float* wsf = reinterpret_cast<const float*>(ws_base);
        map_shadows(P, wsf, shadow, ws_floats, wshadow);
        if (!P.train || table_ok || !P.param_grads)
            if (int r = mark_unread_fp32(P, wsf, ws_floats, tprobs, true)) return r;
    }
    return 0;
}

// The accumulate form's launch lists (m2f_plan_accumulate_grads), built on first use: wg / wg_rest with GF_ACCUM on every problem that
// writes into the gradient buffer.  Then its coverage check: no launch of that backward may OVERWRITE a parameter-gradient range or the
// criterion tail - the backward chain writes the workspace only, every grouped weight-gradient problem accumulates, and the table launch
// and the LayerNorm reduces run their accumulate instantiations.
int build_accumulate(m2f_plan& P) {
    if (P.acc.ready) return 0;
    const float* g0 = P.grads;
    const float* g1 = P.grads + P.pm.total + 4;              // + (loss, den, num) of the criterion tail
    auto in_grads = [&](const void* p) { const float* q = static_cast<const float*>(p); return q && q >= g0 && q < g1; };
    auto accum_copy = [&](const std::vector<Launch>& src, std::vector<Launch>& dst) {
        dst = src;
        for (Launch& l : dst)
            if (l.kind == OP_GEMM)
                for (int i = 0; i < l.gb.count; ++i)
                    if (in_grads(l.gb.pr[i].c) || in_grads(l.gb.pr[i].bias_grad)) l.gb.pr[i].flags |= GF_ACCUM;
    };
    std::vector<Launch> wg_acc, wg_rest_acc;
    if (P.built.wg_table) accum_copy(P.built.wg_rest, wg_rest_acc); else accum_copy(P.built.wg, wg_acc);
    for (const std::vector<Launch>* ls : {&P.built.bwd, &wg_acc, &wg_rest_acc})
        for (const Launch& l : *ls) {
            bool bad = false;
            switch (l.kind) {
                case OP_GEMM:
                    for (int i = 0; i < l.gb.count; ++i) {
                        const GemmProblem& g = l.gb.pr[i];
                        if ((in_grads(g.c) || in_grads(g.bias_grad) || in_grads(g.c8)) && !(g.flags & GF_ACCUM)) bad = true;
                        if ((g.flags & GF_ACCUM) && in_grads(g.c) && (g.flags & GF_NO_F32)) bad = true;
                    }
                    break;
                case OP_ATTN_FWD: case OP_ATTN_BWD:
                    for (int i = 0; i < l.ab.count; ++i) {
                        const AttnProblem& a = l.ab.pr[i];
                        bad = bad || in_grads(a.out) || in_grads(a.probs) || in_grads(a.dq) || in_grads(a.dk) || in_grads(a.dv);
                    }
                    break;
                case OP_LN_FWD: case OP_LN_BWD:
                    for (int i = 0; i < l.lb.count; ++i) {
                        const LnProblem& q = l.lb.pr[i];
                        bad = bad || in_grads(q.out) || in_grads(q.stats) || in_grads(q.dx) || in_grads(q.dx_masked) || in_grads(q.partial);
                    }
                    break;
                case OP_DROPOUT: bad = in_grads(l.dptr) || in_grads(l.dptr2); break;
                default: break;
            }
            if (bad) return fail("m2f_plan_accumulate_grads: coverage check: a launch of the accumulate-form backward would overwrite a parameter-gradient range");
        }
    for (const CastBatch& cb : P.built.wg_casts)
        for (int i = 0; i < cb.count; ++i)
            if (in_grads(cb.it[i].dst) || in_grads(cb.it[i].dst_t)) return fail("m2f_plan_accumulate_grads: coverage check: a cast launch writes into the gradient buffer");
    for (const LnReduceBatch& rb : P.built.lnred)          // (they run their accumulate instantiation: every item must point into the buffer)
        for (int i = 0; i < rb.count; ++i)
            if (!in_grads(rb.it[i].dgamma) || !in_grads(rb.it[i].dbeta)) return fail("m2f_plan_accumulate_grads: coverage check: a LayerNorm reduce writes outside the gradient buffer");
    P.acc.wg.swap(wg_acc); P.acc.wg_rest.swap(wg_rest_acc);
    P.acc.ready = true;
    return 0;
}

// The table's problems with their parameter-shadow pointers (res / gate / ldres / ldgate: the Adam epilogue's; `shadow` may be null) and the
// optimizer-table items the table does NOT cover (1-D parameters, matrices of wg_rest), for the caller to re-tile.  tensor_of[k] = the tensor
// problem k writes, tensor[j] = the tensor of items[j].  Fails when a problem is not a block of one 2-D parameter or a parameter is only
// partly covered.
int table_coverage(m2f_plan& P, uint16_t* param_shadow, std::vector<GemmProblem>& tp, std::vector<int>& tensor_of, std::vector<AdamItem>& items,
                   std::vector<int>& tensor) {
    const ParamTable* t = param_table(P.cfg, true);
    if (!t) return 1;
    // every table problem writes a block of whole rows of ONE 2-D parameter's gradient: find the tensor, its shadows, the first row
    tp = P.built.tprobs_host;
    tensor_of.clear();
    std::vector<long long> covered(t->items.size(), 0);
    for (GemmProblem& q : tp) {
        const long long e = q.c - P.grads;
        const int ti = tensor_at(*t, e);
        if (ti < 0 || t->items[ti].rows == 0 || e >= t->items[ti].off + (long long)t->items[ti].rows * t->items[ti].cols)
            return fail("weight-gradient table coverage: a weight-gradient problem does not write a 2-D parameter's gradient");
        const AdamItem& m = t->items[ti];
        const long long rel = e - m.off;
        // (a block of rows r0.. x columns c0.. of the parameter: whole matrices, the q / k / v row blocks of a fusion layer's in-projection,
        //  the column halves of a Linear over a never-materialised torch.cat)
        const int r0 = (int)(rel / m.cols), c0 = (int)(rel % m.cols), ldd = (m.cols + 7) & ~7, ldt = (m.rows + 7) & ~7;
        if (q.ldc != m.cols || c0 + q.N > m.cols || r0 + q.M > m.rows || q.res || q.gate)
            return fail("weight-gradient table coverage: a weight-gradient problem is not a block of its parameter");
        q.res = param_shadow ? reinterpret_cast<const float*>(param_shadow + m.soff + (size_t)r0 * ldd + c0) : nullptr;
        q.gate = param_shadow ? reinterpret_cast<const float*>(param_shadow + m.soff_t + (size_t)c0 * ldt + r0) : nullptr;
        q.ldres = ldd; q.ldgate = ldt;
        covered[ti] += (long long)q.M * q.N;
        tensor_of.push_back(ti);
    }
    // what is left for the shadow-writing Adam kernel: every item of the optimizer's tensor table except the fully covered matrices
    items.clear(); tensor.clear();
    for (int i = 0; i < t->n(); ++i) {
        const AdamItem& it = t->items[i];
        if (covered[i] == (long long)it.rows * it.cols && it.rows > 0) continue;
        if (covered[i] != 0) return fail("weight-gradient table coverage: a parameter is only partly covered by the weight-gradient table");
        items.push_back(it); tensor.push_back(i);
    }
    if (items.empty() || items.size() > M2F_ADAM_MAX_ITEMS) return fail("weight-gradient table coverage: no / too many residual tensors");
    return 0;
}

}  // namespace m2f
