"""The auxiliary label head (M2FNet.train_step(aux=); csrc/aux_head.hip) at bench geometry C3, bf16 mode, 64 x 16.

Prints one JSON object with "step_ms" for three steps, each train_step + optimizer.step(), alternated in one process and timed with
device events - median, min and max over --reps rounds (at least 5):
  * "plain":     train_step, aux=None - today's launches;
  * "aux":       train_step with aux=(a frozen head of --classes classes, labels, --weight) - the same plan, the rows and tail launches
                 behind the cross-entropy launch and the join launch in the backward;
  * "aux_train": the same with a trainable head - the two parameter-gradient launches too (its own optimizer is not part of the step).
"kernels_ms": the stand-alone call (functional.aux_head: rows, join, parameter gradient) on 1,024 x cls_hidden features, timed the
same way."""
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
from mer_amd.aux_head import AuxiliaryHead  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

MODES = ("plain", "aux", "aux_train")


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
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--classes", type=int, default=3)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    hid = model.m2f_config.cls_hidden
    frozen, hot = AuxiliaryHead(hid, args.classes).to(dev), AuxiliaryHead(hid, args.classes).to(dev)
    frozen.params.requires_grad_(False)
    aux_labels = torch.randint(-1, args.classes, batch[3].shape, generator=torch.Generator().manual_seed(1)).to(dev)
    steps = {"plain": lambda: model.train_step(*batch), "aux": lambda: model.train_step(*batch, aux=(frozen, aux_labels, args.weight)),
             "aux_train": lambda: model.train_step(*batch, aux=(hot, aux_labels, args.weight))}

    def step(mode):
        steps[mode]()
        opt.step()

    for _ in range(2):                                       # every form's graph: warm every mode
        for mode in MODES:
            for _ in range(3):
                step(mode)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(reps):
        for mode in MODES:
            step(mode)                                       # (a change of the switch re-captures: not part of the timed step)
            step(mode)
            times[mode].append(timed(lambda: step(mode)))
    med = {m: statistics.median(v) for m, v in times.items()}
    ce, aux = model.aux_terms()
    g = torch.Generator().manual_seed(2)
    feats = (torch.randn(1024, hid, generator=g).abs() * (torch.rand(1024, hid, generator=g) > 0.4)).to(dev)
    labels = torch.randint(-1, model.m2f_config.cls_out, (1024,), generator=g).to(dev)
    second = torch.randint(-1, args.classes, (1024,), generator=g).to(dev)
    call = lambda: F.aux_head(feats, labels, second, hot.params.detach(), (args.weight, 0.0), None, n_classes=model.m2f_config.cls_out)   # noqa: E731
    for _ in range(3):
        call()
    kern = [timed(call) for _ in range(reps)]
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "weight": args.weight, "classes": args.classes,
           "rounds": reps, "step_ms": {m: {"median": med[m], "min": min(times[m]), "max": max(times[m])} for m in MODES},
           "aux_minus_plain_median": med["aux"] - med["plain"], "aux_train_minus_plain_median": med["aux_train"] - med["plain"],
           "kernels_ms": {"median": statistics.median(kern), "min": min(kern), "max": max(kern), "rows": 1024, "dim": hid},
           "last_ce": float(ce), "last_aux": float(aux)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
