"""The supervised contrastive criterion (M2FNet.train_step(supcon=); csrc/supcon.hip) at bench geometry C3, bf16 mode, 64 x 16.

Prints one JSON object with "step_ms" for two steps, each train_step + optimizer.step(), alternated in one process and timed with
device events - median, min and max over --reps rounds (at least 5):
  * "plain":  train_step, supcon=None - today's launches;
  * "supcon": train_step with supcon=(--weight, --temperature) - the same plan, the contrastive kernels (prep, forward tiles, row
              merge, backward tiles, row gradient, tail) behind the cross-entropy launch and one add launch in the backward.
"kernels_ms": the stand-alone kernels (functional.supcon) on [B * L, cls_hidden] features of the same size, timed the same way."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

MODES = ("plain", "supcon")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--temperature", type=float, default=0.1)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    pair = (args.weight, args.temperature)
    steps = {"plain": lambda: model.train_step(*batch), "supcon": lambda: model.train_step(*batch, supcon=pair)}

    def step(mode):
        steps[mode]()
        opt.step()

    for _ in range(2):                                       # both criteria's graphs: warm every mode
        for mode in MODES:
            for _ in range(3):
                step(mode)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(reps):
        for mode in MODES:
            step(mode)                                       # (a change of criterion re-captures: not part of the timed step)
            step(mode)
            times[mode].append(timed(lambda: step(mode)))
    med = {m: statistics.median(v) for m, v in times.items()}
    ce, con = model.supcon_terms()
    feats = model.last_features().reshape(-1, model.m2f_config.cls_hidden).contiguous()
    labels = batch[3].reshape(-1)
    for _ in range(3):
        F.supcon(feats, labels, None, *pair, n_classes=model.m2f_config.cls_out)
    kern = [timed(lambda: F.supcon(feats, labels, None, *pair, n_classes=model.m2f_config.cls_out)) for _ in range(reps)]
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "weight": args.weight, "temperature": args.temperature,
           "rounds": reps, "step_ms": {m: {"median": med[m], "min": min(times[m]), "max": max(times[m])} for m in MODES},
           "supcon_minus_plain_median": med["supcon"] - med["plain"], "supcon_over_plain": med["supcon"] / med["plain"],
           "kernels_ms": {"median": statistics.median(kern), "min": min(kern), "max": max(kern), "rows": feats.shape[0], "dim": feats.shape[1]},
           "last_ce": float(ce), "last_con": float(con)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
