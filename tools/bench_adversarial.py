"""Adversarial training on the input embeddings (M2FNet.adversarial_step; csrc/adversarial.hip) at bench geometry C3, bf16 mode with fp32
gradients, 64 x 16.

Prints one JSON object with
  * "step_ms": the whole optimizer step in five variants alternated in one process on the same model, timed with device events: "plain"
    (train_step + optimizer.step(), as today), "acc2" / "acc3" (the yardstick: K accumulating micro-batches - train_step(normalise=False)
    under set_grad_accumulation - and one optimizer step with grad_scale = the group's den) and "adv2" / "adv3" (adversarial_step at K = 2
    and 3 with the optimizer).  Median, min and max over --reps rounds, and per K the difference adv - acc: what the K - 1 ascent launches
    per modality and the input-gradient launch of every pass cost beyond K accumulating steps;
  * "alone": the ascent launches alone on the plan's own buffers, --burst back-to-back per timed interval: "ascend_utterance" (per
    modality g, delta and x_clean read, delta and x written: 20 B per element) and "ascend_batch" (the partials launch reads g and delta
    again: 28 B), both modalities per call, with the achieved TB/s - and, from the same run, the SAM perturb kernel's rate (20 B per
    parameter).  An ascent applied many times moves delta many times: the burst is for timing only.
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
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

EPSILON, RHO = 1.0, 0.05


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
    ap.add_argument("--burst", type=int, default=20)
    args = ap.parse_args()
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    eng = model.engine()
    n_params = sum(n for (_, _, n, _) in eng.items)

    def step(mode):
        if mode == "plain":
            loss = model.train_step(*batch)
            opt.step()
            return loss
        k = int(mode[-1])
        if mode.startswith("adv"):
            return model.adversarial_step(*batch, opt, epsilon=EPSILON, steps=k)
        model.set_grad_accumulation(True)
        opt.zero_grad()
        for _ in range(k):
            loss = model.train_step(*batch, normalise=False)
        held, opt.grad_scale = opt.grad_scale, model.loss_terms()[1:2]
        opt.step()
        opt.grad_scale = held
        model.set_grad_accumulation(False)
        return loss

    modes = ("plain", "acc2", "adv2", "acc3", "adv3")
    for mode in modes:                                           # plans, both forms' graphs, the adversarial state: warm all
        for _ in range(3):
            step(mode)
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for _ in range(args.reps):
        for mode in modes:
            times[mode].append(timed(lambda: step(mode)))
    loss = float(step("adv3"))
    delta = model.last_perturbation()
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "parameters": n_params, "epsilon": EPSILON,
           "rounds": args.reps, "loss": loss, "delta_row_norm_mean": {n: float(d.norm(dim=-1).mean()) for n, d in delta.items()},
           "step_ms": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in times.items()}}
    for k in (2, 3):
        out["step_ms"][f"adv{k}_minus_acc{k}_median"] = out["step_ms"][f"adv{k}"]["median"] - out["step_ms"][f"acc{k}"]["median"]

    # the ascent launches alone, on the input gradients of the last pass
    plan = eng.last_adv[0]
    elems = sum(int(d.shape[0] * d.shape[1]) for d in plan.adv_delta.values())
    alone = {}
    for name, kind, per_elem in (("ascend_utterance", 0, 20), ("ascend_batch", 1, 28)):
        def fn():
            for _ in range(args.burst):
                plan.adv_ascend(kind)
        fn()
        torch.cuda.synchronize()
        ts = [timed(fn) / args.burst for _ in range(max(5, args.reps // 3))]
        us = statistics.median(ts) * 1e3
        alone[name] = {"us_median": us, "us_min": min(ts) * 1e3, "us_max": max(ts) * 1e3, "elements": elems, "bytes_per_element": per_elem,
                       "launches": len(plan.adv_delta) * (2 if kind else 1), "TB_per_s": elems * per_elem / (us * 1e-6) / 1e12}
    # ... and the SAM perturb kernel from the same run
    opt.sam_rho = RHO
    model.sam_step(*batch, opt)
    keep = eng.flat.clone()

    def perturb():
        for _ in range(args.burst):
            runtime.sam_perturb(eng.cfg, eng.flat, eng.flat_grad, opt._sam_saved, eng.wshadow, opt._sam_scratch, opt._sam_record, RHO)
    perturb()
    torch.cuda.synchronize()
    ts = [timed(perturb) / args.burst for _ in range(max(5, args.reps // 3))]
    us = statistics.median(ts) * 1e3
    alone["sam_perturb"] = {"us_median": us, "us_min": min(ts) * 1e3, "us_max": max(ts) * 1e3, "bytes_per_parameter": 20,
                            "TB_per_s": n_params * 20 / (us * 1e-6) / 1e12}
    eng.flat.copy_(keep)
    eng.invalidate_shadows()
    opt.sam_rho = None
    out["alone"] = alone
    print(json.dumps(out))


if __name__ == "__main__":
    main()
