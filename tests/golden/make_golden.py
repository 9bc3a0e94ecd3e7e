"""Generate the parity fixtures by running the REAL reference on CPU.

Run in the build container only (needs /root/reference):  python tests/golden/make_golden.py
Imports /root/reference/src/model.py (torch-only module), loads the seeded synthetic weights of
synth.py into it with load_state_dict(strict=True), and records what the reference computes:
eval logits, train-mode (dropout=0.0) loss (plain + class-weighted, the criterion of
src/train.py:48-50), gradients (full for the tiny cases, digests for full-width ones), three
torch.optim.Adam steps (src/train.py:56) and the per-batch metric rule of src/train.py:260-272.
Only tensors (inputs / expected outputs) are written - never reference source or bytecode.
"""
from __future__ import annotations

import os
import pickle
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
import model as ref_model  # noqa: E402  (the reference's src/model.py)


def ns(d):
    return types.SimpleNamespace(**{k: (ns(v) if isinstance(v, dict) else v) for k, v in d.items()})


def real_tables():
    with open(os.path.join(REF, "embeddings/text_base/val.pkl"), "rb") as f:
        t = pickle.load(f)
    with open(os.path.join(REF, "embeddings/audio_wav2vec2/val.pkl"), "rb") as f:
        a = pickle.load(f)
    return t.float().contiguous(), a.float().contiguous()


def run_case(name, out_dir, tables):
    cfg, B, L, lengths, kind = synth.CASES[name]
    sd = synth.make_state_dict(cfg)
    text, audio, key_pad, emotion = synth.make_inputs(cfg, B, L, lengths, kind, real_tables=tables)
    torch.manual_seed(0)
    m = ref_model.M2FNet(ns(cfg))
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert list(m.state_dict().keys()) == list(sd.keys()), "state_dict key ORDER differs from layout.py"

    rec = {}
    if kind == "real":
        rec["text"], rec["audio"] = text.numpy(), audio.numpy()

    m.eval()
    with torch.inference_mode():
        rec["logits_eval"] = m(text, audio, key_pad).numpy()

    # FAM layer-0 intermediates via forward hooks (MHA output, head-averaged weights, layer output)
    if cfg["FAM"]["enabled"] and name in synth.FULL_GRAD_CASES:
        grabbed = {}
        h1 = m.fusion_layers[0].multihead_attention.register_forward_hook(
            lambda mod, i, o: grabbed.update(x=o[0].detach().numpy(), w=o[1].detach().numpy()))
        h2 = m.fusion_layers[0].register_forward_hook(lambda mod, i, o: grabbed.update(y=o.detach().numpy()))
        with torch.no_grad():
            m(text, audio, key_pad)
        h1.remove(), h2.remove()
        rec["fam0_mha_out"], rec["fam0_attn_avg"], rec["fam0_out"] = grabbed["x"], grabbed["w"], grabbed["y"]

    m.train()  # dropout = 0.0 in every case -> deterministic
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    crit_w = torch.nn.CrossEntropyLoss(weight=synth.CLASS_WEIGHTS, ignore_index=-1, label_smoothing=0.1)
    out = m(text, audio, key_pad)
    rec["logits_train"] = out.detach().numpy()
    loss = crit(out.permute(0, 2, 1), emotion)
    rec["loss"] = np.float64(loss.item())
    rec["loss_weighted"] = np.float64(crit_w(out.permute(0, 2, 1), emotion).item())
    m.zero_grad()
    loss.backward()
    specs_done = set()
    norms, dots, names = [], [], []
    for i, (k, p) in enumerate(m.state_dict(keep_vars=True).items()):
        if id(p) in specs_done:
            continue
        specs_done.add(id(p))
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        names.append(k)
        norms.append(float(g.double().norm()))
        dots.append(float((g.double() * synth.digest_vector(tuple(g.shape), 3, i).double()).sum()))
        if (name in synth.FULL_GRAD_CASES and g.numel() <= 32768) or g.dim() == 1 or g.numel() <= 8192:
            rec["grad::" + k] = g.numpy().copy()
    rec["grad_names"] = np.array(names)
    rec["grad_norms"] = np.array(norms)
    rec["grad_dots"] = np.array(dots)

    # weighted-loss gradient digest (checks the class-weight path of the fused CE backward)
    m.zero_grad()
    crit_w(m(text, audio, key_pad).permute(0, 2, 1), emotion).backward()
    rec["gradw::output_last_bias"] = list(m.parameters())[-1].grad.numpy().copy()
    rec["gradw_norm_first"] = np.float64(float(list(m.parameters())[0].grad.double().norm()))

    # three Adam steps on the same batch (coupled L2), lr large enough to be visible
    m.load_state_dict(sd, strict=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        l = crit(m(text, audio, key_pad).permute(0, 2, 1), emotion)
        l.backward()
        opt.step()
        losses.append(l.item())
    rec["adam_losses"] = np.array(losses, dtype=np.float64)
    seen, pn, pd = set(), [], []
    for i, (k, p) in enumerate(m.state_dict(keep_vars=True).items()):
        if id(p) in seen:
            continue
        seen.add(id(p))
        pn.append(float(p.detach().double().norm()))
        pd.append(float((p.detach().double() * synth.digest_vector(tuple(p.shape), 5, i).double()).sum()))
        if name in synth.FULL_GRAD_CASES and p.dim() == 1:
            rec["adam3::" + k] = p.detach().numpy().copy()
    rec["adam3_norms"], rec["adam3_dots"] = np.array(pn), np.array(pd)
    with torch.inference_mode():
        m.eval()
        rec["adam3_logits_eval"] = m(text, audio, key_pad).numpy()
    np.savez_compressed(os.path.join(out_dir, f"{name}.npz"), **rec)
    print(f"{name}: loss {rec['loss']:.6f} weighted {rec['loss_weighted']:.6f} "
          f"adam {losses} -> {os.path.getsize(os.path.join(out_dir, name + '.npz')) / 1e3:.0f} kB")


def c2p_dialogues(n_rows: int, seed: int = 21):
    """MELD-like synthetic dialogue boundaries over n_rows consecutive embedding rows: lengths clamp(round(N(9.6, 5)), 1, 33)
    (MELD: 9.6 utterances per dialogue on average, 33 at most - SURVEY 6), seeded; the last dialogue takes the remainder."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0]))
    lens, left = [], n_rows
    while left > 0:
        n = int(min(max(round(float(g.normal(9.6, 5.0))), 1), 33, left))
        lens.append(n)
        left -= n
    return lens


def c2p_real_val_fixture(out_dir, tables):
    """Shipped depth on REAL embeddings: the reference's config.yaml model VERBATIM (src/config.yaml:31-54:
    768 / 768 / 768, 6 + 6 encoder layers, 5 FAM layers, 2-layer classifier), ALL 1,108 matched rows of
    embeddings/{text_base,audio_wav2vec2}/val.pkl grouped into seeded synthetic dialogues (the MELD CSV with the real
    boundaries is not in the container), batches of 32 dialogues in order (val.data_loader: batch_size 32, no shuffle; last
    batch partial), eval-mode logits of every batch, and the validation rule of src/train.py:245-272: per-batch loss / sklearn
    accuracy / weighted-F1 on the valid utterances, unweighted mean over the batches.

    Weights: synth.make_state_dict (seeded), except the LAST Linear (7 x 768 + 7 values, stored in the fixture): it is fitted
    here - multinomial logistic regression on the reference's own penultimate activations - to seeded labels that are a
    function of the real text embedding (argmax of a seeded projection + MELD's class prior), so that the model separates
    its classes the way a trained head does; a random head leaves half the utterances within 4e-2 of a tie, and a bf16
    score on such a model says nothing about the +-0.2 weighted-F1 target.  The evaluation labels are the clean labels with
    30 % seeded replacements (scores near the 65 % a trained MELD model reaches; every prediction flip moves them)."""
    import yaml
    from sklearn.metrics import accuracy_score, f1_score
    cfg = yaml.safe_load(open(os.path.join(REF, "src/config.yaml")))["model"]
    sd = synth.make_state_dict(cfg)
    torch.manual_seed(0)
    m = ref_model.M2FNet(ns(cfg))
    m.load_state_dict(sd, strict=True)
    m.eval()
    text_tab, audio_tab = tables
    n_rows = text_tab.shape[0]
    assert audio_tab.shape[0] == n_rows
    lens = c2p_dialogues(n_rows)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])

    def batches_of():
        for b0 in range(0, len(lens), 32):
            ls, ss = lens[b0: b0 + 32], starts[b0: b0 + 32]
            B, L = len(ls), max(ls)
            text, audio = torch.zeros(B, L, text_tab.shape[1]), torch.zeros(B, L, audio_tab.shape[1])
            pad = torch.ones(B, L, dtype=torch.bool)
            for i, (n, s0) in enumerate(zip(ls, ss)):
                text[i, :n], audio[i, :n], pad[i, :n] = text_tab[s0: s0 + n], audio_tab[s0: s0 + n], False
            yield ls, ss, text, audio, pad

    # penultimate activations of the reference (input of the last Linear) for every utterance
    feats = np.zeros((n_rows, cfg["CLASSIFIER"]["hidden_size"]), np.float64)
    last = m.output_layer[-1]
    grabbed = {}
    hook = last.register_forward_hook(lambda mod, i, o: grabbed.update(h=i[0].detach()))
    with torch.inference_mode():
        for ls, ss, text, audio, pad in batches_of():
            m(text, audio, pad)
            for i, (n, s0) in enumerate(zip(ls, ss)):
                feats[s0: s0 + n] = grabbed["h"][i, :n].double().numpy()
    hook.remove()
    # seeded, learnable labels with MELD's class prior (paper/MELD.pdf Table 8: neutral 47 %, joy 17, surprise 12, anger 11, sadness 7, disgust 3, fear 3)
    g = np.random.Generator(np.random.Philox(key=[22, 0]))
    prior = np.array([0.47, 0.17, 0.07, 0.11, 0.12, 0.03, 0.03])        # label order of src/utils.py / dataset.py: neutral, joy, sadness, anger, surprise, fear, disgust
    Q = g.standard_normal((text_tab.shape[1], 7)) / np.sqrt(text_tab.shape[1])
    t = text_tab.double().numpy() @ Q
    clean = np.argmax(t / t.std() + np.log(prior), axis=1)
    # multinomial logistic regression (full-batch gradient descent, float64) on the standardised activations
    mu, sg = feats.mean(0), np.full(feats.shape[1], feats.std())      # ONE scale for all features: per-feature scaling would hand
    #                                                                     near-constant activations huge weights (rounding-noise amplifiers)
    X = (feats - mu) / sg
    W, b = np.zeros((7, X.shape[1])), np.zeros(7)
    Y = np.eye(7)[clean]
    for _ in range(200):                                                 # (a partial fit of the clean labels, margins of order 1)
        z = X @ W.T + b
        z -= z.max(1, keepdims=True)
        P = np.exp(z)
        P /= P.sum(1, keepdims=True)
        G = (P - Y) / n_rows
        W -= 0.3 * (G.T @ X + 1e-2 * W)
        b -= 0.3 * G.sum(0)
    W32 = (W / sg).astype(np.float32)
    b32 = (b - (W / sg) @ mu).astype(np.float32)
    sd = dict(sd)
    names = list(sd.keys())
    sd[names[-2]], sd[names[-1]] = torch.from_numpy(W32), torch.from_numpy(b32)
    assert names[-2].endswith(".weight") and tuple(sd[names[-2]].shape) == (7, cfg["CLASSIFIER"]["hidden_size"])
    m.load_state_dict(sd, strict=True)
    labels = clean.copy()
    flip = g.random(n_rows) < 0.30
    labels[flip] = (clean[flip] + g.integers(1, 7, size=int(flip.sum()))) % 7

    flat_logits = np.zeros((n_rows, 7), np.float32)
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    losses, accs, f1s = [], [], []
    with torch.inference_mode():
        for ls, ss, text, audio, pad in batches_of():
            lg = m(text, audio, pad)
            emo = torch.full(pad.shape, -1, dtype=torch.int64)
            for i, (n, s0) in enumerate(zip(ls, ss)):
                flat_logits[s0: s0 + n] = lg[i, :n].numpy()
                emo[i, :n] = torch.from_numpy(labels[s0: s0 + n])
            losses.append(crit(lg.permute(0, 2, 1), emo).item())
            valid = emo != -1
            p, tt = lg.argmax(dim=2)[valid].numpy(), emo[valid].numpy()
            accs.append(accuracy_score(tt, p))
            f1s.append(f1_score(tt, p, average="weighted"))
    pred = flat_logits.argmax(1)
    srt = np.sort(flat_logits, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    rec = {"text_rows": text_tab.numpy(), "audio_rows": audio_tab.numpy(), "lengths": np.array(lens, np.int64),
           "labels": labels.astype(np.int64), "last_weight": W32, "last_bias": b32, "logits": flat_logits,
           "loss_per_batch": np.array(losses), "acc_per_batch": np.array(accs), "f1_per_batch": np.array(f1s),
           "val_loss": np.float64(np.mean(losses)), "acc": np.float64(np.mean(accs)), "f1": np.float64(np.mean(f1s))}
    path = os.path.join(out_dir, "c2p_real_val.npz")
    np.savez_compressed(path, **rec)
    print(f"c2p_real_val: {len(lens)} dialogues / {len(losses)} batches, val loss {rec['val_loss']:.6f} acc {rec['acc']:.6f} "
          f"wF1 {rec['f1']:.6f}; fit of the clean labels {np.mean(pred == clean):.3f}; logit std {flat_logits.std():.2f}, top-2 margin "
          f"min {margin.min():.2e} 1% {np.quantile(margin, 0.01):.3f} median {np.median(margin):.3f}; classes predicted "
          f"{np.bincount(pred, minlength=7).tolist()} -> {os.path.getsize(path) / 1e6:.1f} MB")


def metric_fixture(out_dir):
    """src/train.py:260-272 rule: per-batch sklearn accuracy / weighted-F1, unweighted mean over batches."""
    from sklearn.metrics import accuracy_score, f1_score
    g = np.random.Generator(np.random.Philox(key=[99, 0]))
    rec, accs, f1s = {}, [], []
    for b, (B, L) in enumerate([(32, 16), (32, 12), (7, 9), (5, 3)]):
        logits = g.standard_normal((B, L, 7), dtype=np.float32)
        emo = g.integers(0, 7 if b != 3 else 3, size=(B, L)).astype(np.int64)
        for i in range(B):
            emo[i, int(g.integers(1, L + 1)):] = -1
        pred = torch.argmax(torch.from_numpy(logits), dim=2).numpy()
        msk = emo != -1
        accs.append(accuracy_score(emo[msk], pred[msk]))
        f1s.append(f1_score(emo[msk], pred[msk], average="weighted"))
        rec[f"logits{b}"], rec[f"emotion{b}"] = logits, emo
    rec["acc_per_batch"], rec["f1_per_batch"] = np.array(accs), np.array(f1s)
    rec["acc"], rec["f1"] = np.float64(np.mean(accs)), np.float64(np.mean(f1s))
    np.savez_compressed(os.path.join(out_dir, "metrics.npz"), **rec)
    print("metrics:", rec["acc"], rec["f1"])


def init_fixture(out_dir):
    """Default-init statistics of the reference under manual_seed(0) (init parity of model.py mirrors)."""
    import yaml
    cfg = yaml.safe_load(open(os.path.join(REF, "src/config.yaml")))["model"]
    cfg = dict(cfg, AUDIO=dict(cfg["AUDIO"], n_encoder_layers=1), TEXT=dict(cfg["TEXT"], n_encoder_layers=2),
               FAM=dict(cfg["FAM"], n_layers=1))
    torch.manual_seed(0)
    m = ref_model.M2FNet(ns(cfg))
    rec = {"names": np.array(list(m.state_dict().keys()))}
    rec["sums"] = np.array([float(v.double().sum()) for v in m.state_dict().values()])
    rec["abs_sums"] = np.array([float(v.double().abs().sum()) for v in m.state_dict().values()])
    np.savez_compressed(os.path.join(out_dir, "init_seed0.npz"), **rec)
    print("init fixture:", len(rec["names"]), "tensors")


def default_init_logits_fixture(out_dir):
    """The reference's OWN default init (manual_seed(5), not the synthetic weights) of tiny_odd_heads and its eval logits on
    the synthetic inputs.  The weights themselves are not stored (random, 3 MB): per-tensor digests pin them, and
    tests/test_oracle.py regenerates them with the mirror's default init under the same seed, checks the digests and feeds
    them to the oracle."""
    cfg, B, L, lengths, kind = synth.CASES["tiny_odd_heads"]
    torch.manual_seed(5)
    m = ref_model.M2FNet(ns(cfg)).eval()
    text, audio, key_pad, _ = synth.make_inputs(cfg, B, L, lengths, kind)
    with torch.inference_mode():
        logits = m(text, audio, key_pad)
    sd = m.state_dict()
    vals = [v.double() for v in sd.values()]
    rec = {"names": np.array(list(sd.keys())), "logits_eval": logits.numpy(),
           "sums": np.array([float(v.sum()) for v in vals]), "abs_sums": np.array([float(v.abs().sum()) for v in vals]),
           "dots": np.array([float((v * synth.digest_vector(tuple(v.shape), 9, i).double()).sum()) for i, v in enumerate(vals)])}
    np.savez_compressed(os.path.join(out_dir, "default_init_odd_heads.npz"), **rec)
    print("default-init fixture:", len(sd), "tensors")


if __name__ == "__main__":
    torch.set_num_threads(8)
    tabs = real_tables()
    only = sys.argv[1:]
    for case in synth.CASES:
        if not only or case in only:
            run_case(case, HERE, tabs)
    if not only or "c2p_real_val" in only:
        c2p_real_val_fixture(HERE, tabs)
    if not only:
        metric_fixture(HERE)
        init_fixture(HERE)
    if not only or "default_init_odd_heads" in only:
        default_init_logits_fixture(HERE)
