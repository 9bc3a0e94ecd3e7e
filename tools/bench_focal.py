"""The focal criterion (M2FNet.train_step(focal_gamma=); csrc/rowops.hip m2f_ce_focal_kernel) at bench geometry C3, bf16 mode,
64 dialogues x 16 utterances.

Prints one JSON object with "step_ms" for two steps, each train_step + optimizer.step(), alternated in one process and timed with
device events - median and min over --reps rounds (at least 5), and the medians' difference:
  * "plain": train_step with focal_gamma=None - today's launches;
  * "focal": train_step with focal_gamma=--gamma - the criterion launch alone changes (the same launch count, 4 bytes more read)."""
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

MODES = ("plain", "focal")


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
    ap.add_argument("--gamma", type=float, default=2.0)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    steps = {"plain": lambda: model.train_step(*batch), "focal": lambda: model.train_step(*batch, focal_gamma=args.gamma)}

    def step(mode):
        steps[mode]()
        opt.step()

    for _ in range(2):                                       # the plan and both criteria's graphs: warm every mode
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
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "gamma": args.gamma, "rounds": reps,
           "step_ms": {m: {"median": med[m], "min": min(times[m])} for m in MODES}}
    out["step_ms"]["focal_minus_plain_median"] = med["focal"] - med["plain"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
