"""Times the in-loop wav2vec2 audio encoder (multimodal-emotion-recognition_amd/wav2vec2.py) at wav2vec2-base geometry with
synthetic weights: ms per batch of utterance_embeddings() in fp32 and bf16 mode, for two workloads:
  full    64 utterances x 10 s (160,000 samples each, 499 frames)
  ragged  64 utterances with a MELD-like duration mix (log-normal around 3 s, clipped to 0.5 .. 10 s), padded to the longest
Achieved TFLOP/s use the shape-derived FLOP count of the padded batch (conv stack + positional conv + transformer).

Per-stage split: record a kernel trace of a short run, then let --split read it:
  rocprofv3 --kernel-trace -d DIR -o w2v -- python tools/bench_audio_encoder.py --iters 2 --warmup 1
  python tools/bench_audio_encoder.py --split DIR/.../w2v_results.db [--iters 2 --warmup 1]      (or a *_kernel_trace.csv)
The stages follow the encoder's launch order (wav2vec2.py), so no kernel needs to be recognised by its shape: every call (and every
utterance chunk) starts with m2f_w2v_conv0_stats_kernel; from there up to m2f_w2v_feat_ln_kernel is the conv stack (conv layer 0
and the conv GEMMs), up to m2f_w2v_pos_conv_kernel the feature projection, after it the transformer (encoder LayerNorm, attention,
GEMMs, LayerNorms), and m2f_w2v_masked_mean_kernel the pool; torch's own kernels (length arithmetic, copies) are counted apart.
Calls are taken in the order this script makes them: (fp32, bf16) x (full, ragged), warm-up calls first; warm-ups are dropped.
usage: python tools/bench_audio_encoder.py [--iters 10] [--warmup 3]   -> one JSON line per (workload, precision)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mer_amd  # noqa: F401,E402
from mer_amd.wav2vec2 import Wav2Vec2Encoder, base_config  # noqa: E402


def flops(cfg, N):
    """Forward FLOPs of one utterance padded to N samples (2 per multiply-add)."""
    C, d, Fi, L = cfg["conv_dim"][0], cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    f, n, cin = 0, N, 1
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        n = (n - k) // s + 1
        f += 2 * n * C * cin * k
        cin = C
    S = n
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    conv = f + 2 * S * C * d                                      # (+ feature projection)
    pos = 2 * S * d * (d // G) * K
    tr = L * (2 * S * d * 4 * d + 2 * S * d * 2 * Fi + 4 * S * S * d)
    return conv, pos, tr


def synth(enc, seed=0):
    g = torch.Generator().manual_seed(seed)
    for p in enc.parameters():
        with torch.no_grad():
            if p.dim() == 1:
                p.copy_(1.0 + 0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / np.sqrt(max(1, p[0].numel())))


def read_trace(path):
    """[(kernel name, ms)] in launch order from a rocprofv3 kernel trace: a rocpd database or a *_kernel_trace.csv."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as c:
            rows = c.execute("select name, start, end from kernels order by start").fetchall()
    else:
        import csv
        with open(path) as f:
            rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
        rows.sort(key=lambda r: r[1])
    return [(n, (e - s) / 1e6) for n, s, e in rows]


def stage_split(trace):
    """Per encoder call: {stage: kernel ms}.  A call may hold several utterance chunks; each starts with the conv0 statistics kernel,
    and a call ends with its pool kernel (utterance_embeddings)."""
    calls, cur, phase = [], None, None
    for name, ms in trace:
        if "m2f_w2v_conv0_stats_kernel" in name:
            if cur is None:
                cur = {}
                calls.append(cur)
            phase = "conv_stack"
        if cur is None:
            continue
        if "m2f_w2v_feat_ln_kernel" in name:
            phase = "projection"
        if "m2f_w2v_pos_conv_kernel" in name:
            key = "pos_conv"
            phase = "transformer"
        elif "m2f_w2v_masked_mean_kernel" in name:
            key = "pool"
        elif not name.lstrip().startswith(("void (anonymous namespace)::m2f", "(anonymous namespace)::m2f")):
            key = "torch_misc"
        else:
            key = phase
        cur[key] = cur.get(key, 0.0) + ms
        if "m2f_w2v_masked_mean_kernel" in name:
            cur = None
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--split", default=None, help="kernel trace of an earlier run of this script (same --iters / --warmup): print the stage split")
    args = ap.parse_args()
    if args.split:
        calls = stage_split(read_trace(args.split))
        per = args.warmup + args.iters
        for i, (prec, name) in enumerate([(p, w) for p in ("fp32", "bf16") for w in ("full", "ragged")]):
            timed = calls[i * per + args.warmup: (i + 1) * per]
            keys = sorted({k for c in timed for k in c})
            print(json.dumps({"workload": name, "precision": prec, "calls": len(timed),
                              "kernel_ms_per_call": {k: round(sum(c.get(k, 0.0) for c in timed) / max(1, len(timed)), 3) for k in keys}}))
        return
    cfg = base_config()
    rng = np.random.default_rng(0)
    B = args.batch
    dur = np.clip(rng.lognormal(np.log(3.0), 0.6, size=B), 0.5, 10.0)
    workloads = {"full": [160000] * B, "ragged": [int(x * 16000) for x in dur]}
    for prec in ("fp32", "bf16"):
        enc = Wav2Vec2Encoder(cfg, precision=prec)
        synth(enc)
        enc = enc.cuda().eval()
        for name, lens in workloads.items():
            N = max(lens)
            wave = torch.zeros(B, N)
            for b, n in enumerate(lens):
                wave[b, :n] = 0.1 * torch.randn(n)
            wave, lt = wave.cuda(), torch.tensor(lens).cuda()
            for _ in range(args.warmup):
                enc.utterance_embeddings(wave, lt)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = enc.utterance_embeddings(wave, lt)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            assert torch.isfinite(out).all()
            conv, pos, tr = (B * x for x in flops(cfg, N))
            ms = float(np.median(ts))
            print(json.dumps({"workload": name, "precision": prec, "batch": B, "samples_padded": N, "ms_median": round(ms, 3),
                              "ms_min": round(min(ts), 3), "gflop": round((conv + pos + tr) / 1e9, 1),
                              "gflop_split": {"conv": round(conv / 1e9, 1), "pos_conv": round(pos / 1e9, 1), "transformer": round(tr / 1e9, 1)},
                              "tflops": round((conv + pos + tr) / ms / 1e9, 1)}), flush=True)
        del enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
