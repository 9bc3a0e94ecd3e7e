"""What attention maps cost (M2FNet.last_attention, DialogueStream.attention; csrc/attention_weights.hip and the weights-emitting form of
csrc/attention_stream.hip), at C3 width.

offline  a no-grad forward of B x L dialogues (64 x 16), then per round, alternated:
             forward    - the forward alone: the yardstick
             averaged   - last_attention() for all 17 sites: one gather launch + the result tensors
             per_head   - last_attention(average_heads=False)
stream   a windowed stream (past = history - 1: a ring that stays at `history` live rows however long it runs) of S slots whose rings
         are full, once made with attention=False and once with attention=True; per round, alternated:
             step_off   - stream.step of the stream without attention rows
             step_on    - stream.step of the stream with them (the weights-emitting kernel: one more row of stores per (slot, head))
             rows       - stream.attention() after a step: the averaging launch + the result tensors
Every entry runs --steps calls between one hipEvent pair; median and range over --rounds rounds, us per call.  One JSON line per cell.
    python tools/bench_attention_maps.py --precisions bf16,fp32 --history 16,512"""
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
from bench_streaming import config, timed  # noqa: E402


def stats(xs, digits=1):
    return {"median": round(float(np.median(xs)), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def rounds_of(calls, args):
    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.rounds):                                                   # alternated: drift lands on every entry alike
        for k, fn in calls.items():
            times[k].append(timed(fn, args.steps))
    return {k + "_us": stats(v) for k, v in times.items()}


def offline(args, precision):
    torch.manual_seed(0)
    model = M2FNet(config("c3"), precision=precision).cuda().eval()
    cfg = model.m2f_config
    B, L = args.batch, args.length
    gen = torch.Generator().manual_seed(1)
    text = (torch.randn(B, L, cfg.d_text, generator=gen) * 0.6).cuda()
    audio = (torch.randn(B, L, cfg.d_audio, generator=gen) * 0.2).cuda()
    mask = torch.zeros(B, L, dtype=torch.bool).cuda()
    with torch.inference_mode():
        model(text, audio, mask)
        maps = model.last_attention()
        row = {"part": "offline", "precision": precision, "B": B, "L": L, "sites": len(maps),
               "averaged_bytes": sum(m.numel() * 4 for m in maps.values()),
               "per_head_bytes": sum(m.numel() * 4 for m in model.last_attention(average_heads=False).values()),
               "rounds": args.rounds, "steps_per_round": args.steps}
        row.update(rounds_of({"forward": lambda: model(text, audio, mask), "averaged": model.last_attention,
                              "per_head": lambda: model.last_attention(average_heads=False)}, args))
    print(json.dumps(row), flush=True)


def stream(args, precision, n):
    torch.manual_seed(0)
    model = M2FNet(config("c3"), precision=precision, context=(n - 1, 0)).cuda().eval()
    cfg = model.m2f_config
    S = args.streams
    gen = torch.Generator().manual_seed(1)
    text = (torch.randn(S, n, cfg.d_text, generator=gen) * 0.6).cuda()
    audio = (torch.randn(S, n, cfg.d_audio, generator=gen) * 0.2).cuda()
    with torch.inference_mode():
        off, on = model.stream(S, max_chunk=16), model.stream(S, max_chunk=16, attention=True)
        for st in (off, on):
            st.prefill(text, audio)                                                # the rings are full from here on
        t, a = text[:, 0].contiguous(), audio[:, 0].contiguous()
        on.step(t, a)
        row = {"part": "stream", "precision": precision, "S": S, "history": n, "capacity": on.capacity,
               "rows_bytes": int(on.plan.attn_buf.numel()) * 4, "rounds": args.rounds, "steps_per_round": args.steps}
        row.update(rounds_of({"step_off": lambda: off.step(t, a), "step_on": lambda: on.step(t, a), "rows": on.attention}, args))
        row["on_over_off"] = round(row["step_on_us"]["median"] / row["step_off_us"]["median"], 3)
        off.close()
        on.close()
    print(json.dumps(row), flush=True)
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--history", default="16,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for precision in args.precisions.split(","):
        offline(args, precision)
        for n in (int(x) for x in args.history.split(",")):
            stream(args, precision, n)


if __name__ == "__main__":
    main()
