"""Per-call latency of streaming inference (M2FNet.stream, DialogueStream.step, graph replay) against what a caller does without it: the
context=(None, 0) `forward` over the whole [S, n] prefix to label utterance n.

Grid: S live dialogues in {1, 8, 64}, history n in {1, 16, 64, 512} utterances (the new one included), at C3 width (roberta-large 1024 +
wav2vec2 768) and C2' width (768 / 768; the shipped model section), bf16 and fp32.  One model per (width, precision).  The stream of a
cell is opened under the window (n - 1, 0) with its counts set to n - 1: a ring of n rows, so every timed step reads exactly n live rows
per slot and site - the bytes of a causal step at history n - while the counts grow freely (a causal stream at n = 512 could take one
step only).  Both forms are warmed (plans built, graphs captured); then --rounds rounds of [stream, forward], alternated, each --steps
calls between one hipEvent pair; the reported time is the median over the rounds.  One JSON line per cell, with the byte floor of a
step: the 2-D weights once (2 B in bf16 mode, 4 B in fp32) plus the K / V rows read, at --tbps TB/s.
    python tools/bench_streaming.py --widths c3,c2p --precisions bf16,fp32 --streams 1,8,64 --history 1,16,64,512"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mer_amd  # noqa: E402,F401
from mer_amd import streaming  # noqa: E402
from mer_amd.layout import param_specs  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402


def config(width):
    d_text = {"c3": 1024, "c2p": 768}[width]
    return {"dropout": 0.4,
            "AUDIO": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "TEXT": {"enabled": True, "embedding_size": d_text, "n_head": 8, "n_transformers": 1, "n_encoder_layers": 6},
            "FAM": {"enabled": True, "embedding_size": 768, "n_head": 8, "n_layers": 5},
            "CLASSIFIER": {"hidden_size": 768, "output_size": 7, "n_layers": 2}}


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="c3,c2p")
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--history", default="1,16,64,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--forward-steps", type=int, default=3, help="calls per round of the prefix forward (the slow side)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tbps", type=float, default=6.3, help="HBM bandwidth for the byte floor (measured: 6.3 TB/s)")
    args = ap.parse_args()
    for width in args.widths.split(","):
        for precision in args.precisions.split(","):
            torch.manual_seed(0)
            model = M2FNet(config(width), precision=precision, context=(None, 0)).cuda().eval()
            cfg = model.m2f_config
            bf16 = precision == "bf16"
            w_bytes = sum(s.numel for s in param_specs(cfg)[0] if not s.alias_of and len(s.shape) == 2) * (2 if bf16 else 4)
            gen = torch.Generator().manual_seed(1)
            for S in (int(x) for x in args.streams.split(",")):
                for n in (int(x) for x in args.history.split(",")):
                    text = (torch.randn(S, n, cfg.d_text, generator=gen) * 0.6).cuda()
                    audio = (torch.randn(S, n, cfg.d_audio, generator=gen) * 0.2).cuda()
                    mask = torch.zeros(S, n, dtype=torch.bool, device="cuda")
                    new_t, new_a = text[:, -1].contiguous(), audio[:, -1].contiguous()
                    with torch.inference_mode():
                        model.set_context(n - 1, 0)
                        st = model.stream(S)
                        model.set_context(None, 0)
                        st.plan.len.fill_(n - 1)
                        st.lengths = [n - 1] * S
                        stream_call = lambda: st.step(new_t, new_a)                    # noqa: E731
                        forward_call = lambda: model(text, audio, mask)                # noqa: E731
                        for _ in range(args.warmup):
                            stream_call()
                            forward_call()
                        torch.cuda.synchronize()
                        ts, tf = [], []
                        for _ in range(args.rounds):                                   # alternated: drift lands on both forms alike
                            ts.append(timed(stream_call, args.steps))
                            tf.append(timed(forward_call, args.forward_steps))
                    kv_bytes = streaming.cache_bytes(cfg, S, n, bf16=bf16)
                    floor = (w_bytes + kv_bytes) / (args.tbps * 1e12) * 1e6
                    ms, mf = float(np.median(ts)), float(np.median(tf))
                    print(json.dumps({"width": width, "precision": precision, "S": S, "n": n, "launches_per_step": st.plan.num_launches(),
                                      "stream_us": {"median": round(ms, 1), "min": round(min(ts), 1), "max": round(max(ts), 1)},
                                      "prefix_forward_us": {"median": round(mf, 1), "min": round(min(tf), 1), "max": round(max(tf), 1)},
                                      "ratio": round(mf / ms, 2), "weight_bytes": w_bytes, "kv_bytes_read": kv_bytes,
                                      "byte_floor_us": round(floor, 1), "rounds": args.rounds, "steps_per_round": args.steps}), flush=True)
                    st.close()
                    for k in list(model.engine().plans):                               # the prefix plans of this cell: gigabytes at n = 512
                        model.engine().plans.pop(k).close()
                    torch.cuda.empty_cache()
            del model
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
