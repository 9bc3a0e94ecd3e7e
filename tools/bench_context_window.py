"""What a context band costs and saves (M2FNet(context=(past, future))): bf16 train steps with full attention, causal (None, 0)
and a window of 8 (8, 0), alternated, on
  long   the long-dialogue set of tools/long_dialogue_step.py (C2' width, 16 dialogues of 8..110 utterances: packed plan,
         long-dialogue attention kernels, two 64-row blocks per dialogue);
  l512   the same model on 4 dialogues of 512 utterances (eight blocks: causal skips 28 of the 64 block pairs, (8, 0) 49);
  c3     BASELINE C3 (roberta-large 1024 + wav2vec2 768, 64 dialogues x 16 utterances: the short kernels, which skip nothing).
Every model is built and warmed (graph captured) first; then --rounds rounds of [full, causal, window], each --steps replayed steps
between one hipEvent pair; the reported time of a form is the median over the rounds.  One JSON line per workload.
    python tools/bench_context_window.py --workloads long,l512,c3 --rounds 7 --steps 20
--kernel-stats FORM (full | causal | window): only replays that form's step --steps times on ONE workload, for a separate run under
`rocprofv3 --kernel-trace --stats -d DIR -o p -- python tools/bench_context_window.py --workloads long --kernel-stats causal`
(the m2f_attn_dlong_* rows of p_kernel_stats.csv are the long-dialogue kernels' times)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
import long_dialogue_step as lds  # noqa: E402

FORMS = {"full": (None, None), "causal": (None, 0), "window": (8, 0)}


def c3_config():
    return {"dropout": 0.4,
            "AUDIO": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "TEXT": {"enabled": True, "embedding_size": 1024, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "FAM": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_layers": 5},
            "CLASSIFIER": {"hidden_size": 768, "output_size": 7, "n_layers": 2}}


def full_batch(B, L, d_text, d_audio, seed=0):
    gen = torch.Generator().manual_seed(seed)
    text = torch.randn(B, L, d_text, generator=gen) * 0.6
    audio = torch.randn(B, L, d_audio, generator=gen) * 0.2
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    emotion = torch.randint(0, 7, (B, L), generator=gen)
    return [t.cuda() for t in (text, audio, key_pad, emotion)]


def workload(name):
    if name == "long":
        return lds.config(), lds.batch()[0]
    if name == "l512":
        return lds.config(), full_batch(4, 512, 768, 768)
    if name == "c3":
        return c3_config(), full_batch(64, 16, 1024, 768)
    raise SystemExit(f"unknown workload {name!r} (long, l512, c3)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="long,l512,c3")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-stats", choices=sorted(FORMS), default=None)
    args = ap.parse_args()
    names = args.workloads.split(",")
    if args.kernel_stats and len(names) != 1:
        raise SystemExit("--kernel-stats takes one workload")
    for name in names:
        cfg, batch = workload(name)
        forms = [args.kernel_stats] if args.kernel_stats else list(FORMS)
        models = {}
        for f in forms:
            torch.manual_seed(0)
            models[f] = M2FNet(cfg, precision=args.precision, context=FORMS[f]).cuda().train()
            for _ in range(args.warmup):
                loss = models[f].train_step(*batch, use_graph=True)
            assert torch.isfinite(loss), (name, f)
        torch.cuda.synchronize()
        if args.kernel_stats:
            for _ in range(args.steps):
                models[forms[0]].train_step(*batch, use_graph=True)
            torch.cuda.synchronize()
            print(json.dumps({"workload": name, "form": forms[0], "context": FORMS[forms[0]], "steps": args.steps}))
            continue
        times = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f in forms:                                 # alternated: drift of the machine lands on every form alike
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    models[f].train_step(*batch, use_graph=True)
                e1.record()
                torch.cuda.synchronize()
                times[f].append(e0.elapsed_time(e1) / args.steps)
        pl = next(iter(models[forms[0]].engine().plans.values()))
        print(json.dumps({"workload": name, "precision": args.precision, "plan": {"B": pl.B, "L": pl.L, "T": pl.T, "packed": bool(pl.packed)},
                          "rounds": args.rounds, "steps_per_round": args.steps,
                          "ms_per_step": {f: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                                          for f, t in times.items()}}))
        del models
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
