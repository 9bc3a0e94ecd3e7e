"""What it costs to load an n-utterance history into S stream slots (M2FNet.stream, DialogueStream), three ways:
  * `prefill` through the chunk plan, T = 16 and T = 64 utterances per slot and call (ceil(n / T) captured graphs of S * T rows each);
  * n `step` calls (one launch-bound row per dialogue each) - all a stream could do before it had a chunk plan;
  * the context=(None, 0) `forward` over the same [S, n] prefix, which computes the same K / V rows and fills no cache (the yardstick).

Grid: C3 width (roberta-large 1024 + wav2vec2 768), bf16 and fp32, S in {1, 8, 64}, n in {16, 64, 512}.  One model per precision; a
cell's streams are causal with a capacity of n rows, so the history fills them to the last row.  Every form is warmed (plans built,
graphs captured); then --rounds rounds of [prefill T=16, prefill T=64, n steps, forward], alternated so that drift lands on all forms
alike, each form's calls between one hipEvent pair (the `reset()` in front of a load is inside the pair: one small launch).  The
reported time is the median over the rounds, in microseconds per history load.  One JSON line per cell.  No threshold.
    python tools/bench_stream_prefill.py --precisions bf16,fp32 --streams 1,8,64 --history 16,64,512"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
from bench_streaming import config, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", default="c3")
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--history", default="16,64,512")
    ap.add_argument("--chunks", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loads", type=int, default=3, help="history loads per round of the prefill and forward forms")
    ap.add_argument("--step-loads", type=int, default=1, help="... of the n-steps form (the slow side)")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    chunks = [int(x) for x in args.chunks.split(",")]
    for precision in args.precisions.split(","):
        torch.manual_seed(0)
        model = M2FNet(config(args.width), precision=precision, context=(None, 0)).cuda().eval()
        cfg = model.m2f_config
        gen = torch.Generator().manual_seed(1)
        for S in (int(x) for x in args.streams.split(",")):
            for n in (int(x) for x in args.history.split(",")):
                text = (torch.randn(S, n, cfg.d_text, generator=gen) * 0.6).cuda()
                audio = (torch.randn(S, n, cfg.d_audio, generator=gen) * 0.2).cuda()
                mask = torch.zeros(S, n, dtype=torch.bool, device="cuda")
                cols = [(text[:, i].contiguous(), audio[:, i].contiguous()) for i in range(n)]
                with torch.inference_mode():
                    streams = {T: model.stream(S, capacity=n, max_chunk=T) for T in chunks}
                    stepper = streams[chunks[0]]

                    def load(T):
                        streams[T].reset()
                        streams[T].prefill(text, audio)

                    def steps():
                        stepper.reset()
                        for t, a in cols:
                            stepper.step(t, a)

                    forms = [(f"prefill_T{T}", (lambda T=T: load(T)), args.loads) for T in chunks]
                    forms += [("steps", steps, args.step_loads), ("prefix_forward", lambda: model(text, audio, mask), args.loads)]
                    for _ in range(args.warmup):
                        for _, fn, _ in forms:
                            fn()
                    torch.cuda.synchronize()
                    times = {name: [] for name, _, _ in forms}
                    for _ in range(args.rounds):                                       # alternated: drift lands on every form alike
                        for name, fn, reps in forms:
                            times[name].append(timed(fn, reps))
                row = {"width": args.width, "precision": precision, "S": S, "n": n, "rounds": args.rounds,
                       "launches_per_chunk_call": {f"T{T}": streams[T].chunk_plan.num_launches() for T in chunks},
                       "launches_per_step": stepper.plan.num_launches()}
                for name, ts in times.items():
                    row[name + "_us"] = {"median": round(float(np.median(ts)), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
                best = min(row[f"prefill_T{T}_us"]["median"] for T in chunks)
                row["steps_over_best_prefill"] = round(row["steps_us"]["median"] / best, 2)
                row["best_prefill_over_forward"] = round(best / row["prefix_forward_us"]["median"], 2)
                print(json.dumps(row), flush=True)
                for st in streams.values():
                    st.close()
                for k in list(model.engine().plans):                                   # the prefix plans of this cell
                    model.engine().plans.pop(k).close()
                torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
