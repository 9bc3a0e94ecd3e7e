"""The distillation criterion (M2FNet.train_step(teacher_logits=, distill=); csrc/rowops.hip m2f_ce_distill_kernel) at bench geometry
C3, bf16 mode, 64 dialogues x 16 utterances.

Prints one JSON object with "step_ms" for three steps, each train_step + optimizer.step(), alternated in one process and timed with
device events - median and min over --reps rounds (at least 5), and the medians' differences to "plain":
  * "plain":     the hard-label train_step;
  * "distilled": train_step with teacher logits that are already there (cached with the dataset) - the criterion launch alone changes;
  * "distiller": Distiller.train_step - the teacher's eval forward (an offline model of the same geometry) in front of it.
The student is causal (context = (None, 0)), the teacher offline."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mer_amd  # noqa: E402,F401
from mer_amd.distill import Distiller  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

MODES = ("plain", "distilled", "distiller")


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
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=2.0)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    student = M2FNet(wl["cfg"], precision="bf16", context=(None, 0)).to(dev).train()
    teacher = M2FNet(wl["cfg"], precision="bf16").to(dev)
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(student, lr=1e-4, weight_decay=0.01)
    d = Distiller(student, teacher, alpha=args.alpha, temperature=args.temperature)
    cached = d.teacher_logits(batch[0], batch[1], batch[2]).clone()
    pair = (args.alpha, args.temperature)

    steps = {
        "plain": lambda: student.train_step(*batch),
        "distilled": lambda: student.train_step(*batch, teacher_logits=cached, distill=pair),
        "distiller": lambda: d.train_step(*batch),
    }

    def step(mode):
        steps[mode]()
        opt.step()

    for _ in range(2):                                       # plans, both criteria's graphs, the teacher's plan: warm every mode
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
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "alpha": args.alpha, "temperature": args.temperature,
           "rounds": reps, "step_ms": {m: {"median": med[m], "min": min(times[m])} for m in MODES}}
    out["step_ms"]["distilled_minus_plain_median"] = med["distilled"] - med["plain"]
    out["step_ms"]["distiller_minus_plain_median"] = med["distiller"] - med["plain"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
