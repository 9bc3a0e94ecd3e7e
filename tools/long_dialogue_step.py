"""Train-step time on long, ragged dialogues (IEMOCAP-like: whole recorded sessions of up to ~110 utterances).

C2'-width model (the shipped config.yaml: 768 / 768 / 768, 8 heads, 6 encoder layers per modality, 5 fusion layers, dropout 0.4),
16 dialogues with seeded lengths uniform over 8..110.  The batch's longest dialogue exceeds 64 utterances, so M2FNet runs it on a
packed plan with the long-dialogue attention kernels.  Prints one JSON line: ms per step and valid utterances per second.
    python tools/long_dialogue_step.py --precision bf16 --steps 50 --warmup 10
Kernel shares: run it under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/long_dialogue_step.py ...`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402


def config():
    return {"dropout": 0.4,
            "AUDIO": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "TEXT": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "FAM": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_layers": 5},
            "CLASSIFIER": {"hidden_size": 768, "output_size": 7, "n_layers": 2}}


def batch(B=16, lo=8, hi=110, seed=0, device="cuda"):
    g = np.random.Generator(np.random.Philox(key=[seed, 0]))
    lens = g.integers(lo, hi + 1, size=B)
    lens[0] = hi                                              # the longest dialogue of the batch is at the top of the range
    L = int(lens.max())
    gen = torch.Generator().manual_seed(seed)
    text = torch.randn(B, L, 768, generator=gen) * 0.6
    audio = torch.randn(B, L, 768, generator=gen) * 0.2
    key_pad = torch.arange(L)[None, :] >= torch.from_numpy(lens)[:, None]
    emotion = torch.randint(0, 7, (B, L), generator=gen).masked_fill(key_pad, -1)
    text[key_pad] = 0
    audio[key_pad] = 0
    return [t.to(device) for t in (text, audio, key_pad, emotion)], lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    m = M2FNet(config(), precision=a.precision).cuda().train()
    (text, audio, key_pad, emotion), lens = batch()
    use_graph = not a.no_graph
    for _ in range(a.warmup):
        m.train_step(text, audio, key_pad, emotion, use_graph=use_graph)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            loss = m.train_step(text, audio, key_pad, emotion, use_graph=use_graph)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / a.steps)
    pl = next(iter(m.engine().plans.values()))
    ms = float(np.median(times))
    print(json.dumps({"workload": "C2' width, 16 dialogues of 8..110 utterances", "precision": a.precision, "graph": use_graph,
                      "plan": {"B": pl.B, "L": pl.L, "T": pl.T, "packed": bool(pl.packed)}, "valid_utterances": int(lens.sum()),
                      "ms_per_step": round(ms, 3), "ms_per_step_repeats": [round(t, 3) for t in times],
                      "utterances_per_s": round(float(lens.sum()) / ms * 1e3, 1), "loss": float(loss.item())}))


if __name__ == "__main__":
    main()
