"""Cost of input gradients: the autograd forward + criterion + backward of M2FNet (not the fused train_step) at the BASELINE
geometries, in three modes - parameter gradients only (as before), parameter and input gradients, input gradients only (frozen
model: requires_grad_(False)).  Per step: a hipEvent pair (torch.cuda.Event) around forward + loss + backward on the current
stream, after a warm-up; prints ms per step (median, mean) and the backward launch count of the plan each mode runs on.

    python tools/bench_input_grads.py [--workloads c3,c2] [--dtype bf16] [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mer_amd  # noqa: E402,F401
from bench import WORKLOADS, synthetic_batch  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

MODES = {"params": (True, False), "params+inputs": (True, True), "inputs": (False, True)}


def run(wl, dtype, steps, warmup):
    w = WORKLOADS[wl]
    torch.manual_seed(0)
    model = M2FNet(w["cfg"], precision=dtype).cuda().train()
    text, audio, mask, emotion = synthetic_batch(w["cfg"], w["B"], w["L"], 0, "cuda")
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    out = {}
    for mode, (params, inputs) in MODES.items():
        model.requires_grad_(params)
        times = []
        for i in range(warmup + steps):
            t = text.detach().requires_grad_(inputs)
            a = audio.detach().requires_grad_(inputs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            crit(model(t, a, mask).permute(0, 2, 1), emotion).backward()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
        plan = list(model.engine().plans.values())[-1]          # the plan this mode ran on (most recently used)
        out[mode] = {"ms_median": round(statistics.median(times), 4), "ms_mean": round(statistics.mean(times), 4),
                     "bwd_launches": plan.num_launches()["backward"], "input_mask": plan.input_mask,
                     "param_grads": plan.param_grads}
        print(f"{wl} {dtype} {mode:14s} {out[mode]['ms_median']:8.3f} ms/step (mean {out[mode]['ms_mean']:.3f}), "
              f"{out[mode]['bwd_launches']} backward launches", flush=True)
    model.requires_grad_(True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c2")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    res = {wl: run(wl, a.dtype, a.steps, a.warmup) for wl in a.workloads.split(",")}
    print(json.dumps({"bench_input_grads": res, "dtype": a.dtype, "steps": a.steps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
