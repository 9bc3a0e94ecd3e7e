"""The R-Drop criterion (M2FNet.train_step(rdrop=); csrc/rowops.hip m2f_ce_rdrop_kernel) at bench geometry C3, bf16 mode, 64 x 16.

Prints one JSON object with "step_ms" for three steps, each train_step + optimizer.step(), alternated in one process and timed with
device events - median, min and max over --reps rounds (at least 5):
  * "plain_64":  train_step on 64 dialogues, rdrop=None - today's launches;
  * "plain_128": train_step on 128 dialogues (the batch twice), rdrop=None - the plan the R-Drop step runs, under the plain criterion;
  * "rdrop_64":  train_step on 64 dialogues with rdrop=--alpha - that 128-dialogue plan, the batch copied twice into it, the R-Drop
                 criterion in the plain one's place and one more reduce launch.
The R-Drop step's cost is to be read against plain_128 of the same run ("rdrop_minus_plain_128_median"), and against two plain
64-dialogue steps ("rdrop_over_plain_64")."""
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

MODES = ("plain_64", "plain_128", "rdrop_64")


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
    ap.add_argument("--alpha", type=float, default=1.0)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    twice = [torch.cat([x, x], 0) for x in batch]
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    steps = {"plain_64": lambda: model.train_step(*batch), "plain_128": lambda: model.train_step(*twice),
             "rdrop_64": lambda: model.train_step(*batch, rdrop=args.alpha)}

    def step(mode):
        steps[mode]()
        opt.step()

    for _ in range(2):                                       # both plans and both criteria's graphs: warm every mode
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
    ce, kl = model.rdrop_terms()
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "alpha": args.alpha, "rounds": reps,
           "step_ms": {m: {"median": med[m], "min": min(times[m]), "max": max(times[m])} for m in MODES},
           "rdrop_minus_plain_128_median": med["rdrop_64"] - med["plain_128"], "rdrop_over_plain_64": med["rdrop_64"] / med["plain_64"],
           "last_ce": float(ce), "last_kl": float(kl)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
