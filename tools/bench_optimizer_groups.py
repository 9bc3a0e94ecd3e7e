"""Parameter groups and decoupled weight decay (FusedAdam(params=[...]) / FusedAdamW) at bench geometry C3, bf16 mode: what the grouped
kernels cost against today's single coupled group.

Forms, each its own optimizer on the SAME model:
  a  today's single coupled group                FusedAdam(model)                          (today's kernels and entries)
  b  one decoupled group                         FusedAdamW(model)
  c  AdamW, no decay on 1-D tensors, both encoders at 0.1 x lr   (four groups)
  d  both encoders in no group                   FusedAdamW(model, params=<everything else>)
Prints one JSON object with, for fp32 gradients and for bf16 gradients (M2FNet.set_grad_bf16):
  * "step_ms": the whole step - train_step + optimizer.step() - of a, b, c, d alternated step by step in one process, timed with device
    events: median, min and max over --reps rounds;
  * "in_step_ms" (fp32 gradients only; a, b, c): the optimizer INSIDE the step (train_step(optimizer=...)).  Changing the optimizer
    re-arms the plan and re-captures its graph, so these alternate in blocks: per round and form two untimed steps, then --block timed
    ones; median, min and max of the per-step times over all rounds.
--kernel-stats FORM [--gradients fp32 | bf16] [--in-step]: only runs --reps whole steps of that form, for a separate run under
  rocprofv3 --kernel-trace --stats (the optimizer kernels' own time inside the step); prints nothing else.
Fails without a device."""
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
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

FORMS = ("a", "b", "c", "d")
ENCODERS = ("audio_encoders", "text_encoders")
LR, WD = 1e-4, 0.01


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def optimizers(model):
    named = list(model.named_parameters())
    groups_c = {}
    for n, p in named:
        groups_c.setdefault((n.startswith(ENCODERS), p.dim() == 1), []).append(p)
    c = [{"params": ps, "lr": LR * (0.1 if enc else 1.0), "weight_decay": 0.0 if one_d else WD} for (enc, one_d), ps in groups_c.items()]
    return {"a": FusedAdam(model, lr=LR, weight_decay=WD),
            "b": FusedAdamW(model, lr=LR, weight_decay=WD),
            "c": FusedAdamW(model, lr=LR, weight_decay=WD, params=c),
            "d": FusedAdamW(model, lr=LR, weight_decay=WD, params=[p for n, p in named if not n.startswith(ENCODERS)])}


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--kernel-stats", choices=FORMS, default=None)
    ap.add_argument("--in-step", action="store_true", help="with --kernel-stats: the optimizer inside the step")
    ap.add_argument("--gradients", choices=["fp32", "bf16"], default=None, help="only this gradient precision (default: both)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizer_groups: needs an MI355X (gfx950) device")
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opts = optimizers(model)
    eng = model.engine()
    n_params = sum(n for (_, _, n, _) in eng.items)
    owned = {f: sum(n for (p, _, n, _), g in zip(eng.items, o.tensor_group_map()) if g >= 0) for f, o in opts.items()}

    def step(form):
        model.train_step(*batch)
        opts[form].step()

    def in_step(form):
        model.train_step(*batch, optimizer=opts[form])

    out = {"workload": wl["name"], "precision": "bf16", "parameters": n_params, "owned_parameters": owned,
           "groups": {f: len(o.param_groups) for f, o in opts.items()}}
    for grads in ("fp32", "bf16"):
        if args.gradients and grads != args.gradients:
            continue
        assert model.set_grad_bf16(grads == "bf16") == (grads == "bf16")
        if args.kernel_stats:
            fn = in_step if args.in_step else step
            for _ in range(3 + args.reps):
                fn(args.kernel_stats)
            torch.cuda.synchronize()
            continue
        for form in FORMS:                                      # plans, graphs, tables: warm every form
            for _ in range(3):
                step(form)
        torch.cuda.synchronize()
        times = {f: [] for f in FORMS}
        for _ in range(args.reps):
            for form in FORMS:
                times[form].append(timed(lambda: step(form)))
        res = {"step_ms": {f: summary(times[f]) for f in FORMS}, "rounds": args.reps}
        if grads == "fp32":
            itimes = {f: [] for f in "abc"}
            armed = {}
            for _ in range(max(2, args.reps // args.block)):
                for form in "abc":
                    in_step(form)
                    in_step(form)
                    torch.cuda.synchronize()
                    plan = next(p for p in eng.plans.values() if p.train)
                    armed[form] = getattr(plan, "_fused_key", None) is not None
                    itimes[form] += [timed(lambda: in_step(form)) for _ in range(args.block)]
            res["in_step_ms"] = {f: dict(summary(itimes[f]), armed=armed[f]) for f in "abc"}
        out[grads + "_gradients"] = res
    if not args.kernel_stats:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
