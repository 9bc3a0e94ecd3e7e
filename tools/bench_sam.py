"""Sharpness-aware minimisation (FusedAdam(sam_rho=...), M2FNet.sam_step; csrc/sam.hip) at bench geometry C3, bf16 mode, 64 x 16.

Prints one JSON object with
  * "step_ms": the whole optimizer step in two variants alternated in one process on the same model, timed with device events:
    "plain" (train_step + optimizer.step(), sam_rho None) and "sam" (M2FNet.sam_step: two passes, the perturbation, the restore, the
    update).  Median, min and max over --reps rounds, and the ratio of the medians;
  * "alone": the launches alone, --burst back-to-back per timed interval so that the event pair's own overhead is amortised, with the
    bytes each moves per parameter and the achieved TB/s: "perturb" (w and g read, w and the backup written, the two bf16 shadows
    written: 20 B with fp32 gradients), "restore" (the backup read, w written: 8 B), "norm" (the sum of squares + the finalize launch: g
    read, 4 B) and, from the same run, the shadow-writing Adam kernel (p, m, v read and written, g read, the shadows written: 32 B).
    A perturbation applied twice moves w twice: the burst is for timing only, the model is restored behind it.
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

RHO = 0.05


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
        if mode == "sam":
            opt.sam_rho = RHO
            return model.sam_step(*batch, opt)
        opt.sam_rho = None
        loss = model.train_step(*batch)
        opt.step()
        return loss

    for mode in ("plain", "sam"):                                # plans, graphs, the backup buffer: warm both
        for _ in range(3):
            step(mode)
    torch.cuda.synchronize()
    assert eng.shadows_fresh()
    times = {"plain": [], "sam": []}
    for _ in range(args.reps):
        for mode in times:
            times[mode].append(timed(lambda: step(mode)))
    loss = float(step("sam"))
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "parameters": n_params, "rho": RHO, "rounds": args.reps,
           "loss": loss, "sam_grad_norm": float(opt.sam_norm()),
           "step_ms": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in times.items()}}
    out["step_ms"]["sam_over_plain_median"] = out["step_ms"]["sam"]["median"] / out["step_ms"]["plain"]["median"]

    # the launches alone, on the gradient of the last step
    grad = eng.flat_grad
    saved, scratch, record = opt._sam_saved, opt._sam_scratch, opt._sam_record
    keep = eng.flat.clone()

    def perturb():
        for _ in range(args.burst):
            runtime.sam_perturb(eng.cfg, eng.flat, grad, saved, eng.wshadow, scratch, record, RHO)

    def restore():
        for _ in range(args.burst):
            runtime.sam_restore(eng.cfg, eng.flat, saved)

    def norm():
        for _ in range(args.burst):
            runtime.grad_sumsq(eng.cfg, grad, scratch)

    def adam():
        opt.sam_rho = None
        for _ in range(args.burst):
            opt.step()

    alone = {}
    for name, fn, per_param in (("perturb", perturb, 20), ("restore", restore, 8), ("norm", norm, 4), ("adam_shadowed", adam, 32)):
        fn()
        torch.cuda.synchronize()
        ts = [timed(fn) / args.burst for _ in range(max(5, args.reps // 3))]
        us = statistics.median(ts) * 1e3
        alone[name] = {"us_median": us, "us_min": min(ts) * 1e3, "us_max": max(ts) * 1e3, "bytes_per_parameter": per_param,
                       "TB_per_s": n_params * per_param / (us * 1e-6) / 1e12}
        if name in ("perturb", "restore"):                       # (the finalize launch rides in every perturb call: one workgroup)
            eng.flat.copy_(keep)
            eng.invalidate_shadows()
    alone["perturb_over_adam_TB_per_s"] = alone["perturb"]["TB_per_s"] / alone["adam_shadowed"]["TB_per_s"]
    out["alone"] = alone
    print(json.dumps(out))


if __name__ == "__main__":
    main()
