"""Gradient accumulation over micro-batches (M2FNet.set_grad_accumulation) at bench geometry C3, bf16 mode with fp32 gradients.

Prints one JSON object:
  * "micro_batch_ms": forward + criterion + backward of one C3 batch in the overwrite form and in the accumulate form, the two
    alternated in one process on the same plan (each form replays its own captured graph), timed with device events - median and
    min over --reps pairs, and the difference;
  * "throughput": utterances/s for k in {1, 2, 4, 8} micro-batches of 64 x 16 per optimizer step (train_step(normalise=False) k
    times, then FusedAdam with grad_scale = the group's den): --windows timed windows of --groups groups per k, the k values
    interleaved window by window (one warm-up group each first); min / median / max over the windows.
--kernel-stats FORM (overwrite | accumulate): only replays that form's step --reps times, for a separate run under
  rocprofv3 --kernel-trace --stats (the table launch's kernel time in each form), and prints nothing else.
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
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--kernel-stats", choices=["overwrite", "accumulate"], default=None)
    args = ap.parse_args()
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    text, audio, mask, emotion = batch
    model.train_step(text, audio, mask, emotion, normalise=False)          # plans, shadows, warm-up
    eng = model.engine()
    plan = next(p for p in eng.plans.values() if p.train)

    def step(acc):
        plan.accumulate_grads(acc)
        with torch.cuda.stream(eng.stream):
            plan.step(0.1, False, False, True)

    if args.kernel_stats:
        acc = args.kernel_stats == "accumulate"
        for _ in range(3):
            step(acc)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            step(acc)
        torch.cuda.synchronize()
        return
    for _ in range(5):                                                       # capture both graphs, warm both
        step(False)
        step(True)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(args.reps):
        for acc in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(eng.stream)
            step(acc)
            e1.record(eng.stream)
            e1.synchronize()
            times[acc].append(e0.elapsed_time(e1))
    plan.accumulate_grads(False)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"workload": wl["name"], "precision": "bf16", "gradients": "fp32",
           "micro_batch_ms": {"overwrite_median": med[False], "accumulate_median": med[True],
                              "overwrite_min": min(times[False]), "accumulate_min": min(times[True]),
                              "accumulate_minus_overwrite_median": med[True] - med[False], "pairs": args.reps}}
    # utterances/s with k micro-batches per optimizer step
    model.set_grad_accumulation(True)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    utt = wl["B"] * wl["L"]
    ks = (1, 2, 4, 8)

    def group(k):
        opt.zero_grad()
        for _ in range(k):
            model.train_step(text, audio, mask, emotion, normalise=False)
        opt.grad_scale = model.loss_terms()[1:2]
        opt.step()

    for k in ks:
        group(k)
    torch.cuda.synchronize()
    rates = {k: [] for k in ks}
    for _ in range(args.windows):
        for k in ks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.groups):
                group(k)
            e1.record()
            e1.synchronize()
            rates[k].append(utt * k * args.groups / (e0.elapsed_time(e1) / 1e3))
    out["throughput"] = {str(k): {"utt_per_s_min": min(v), "utt_per_s_median": statistics.median(v), "utt_per_s_max": max(v),
                                  "windows": args.windows, "groups_per_window": args.groups} for k, v in rates.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
