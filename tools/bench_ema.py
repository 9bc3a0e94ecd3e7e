"""The weight average inside the optimizer kernels (FusedAdam(ema_decay=...), csrc/adam.hip) at bench geometry C3, bf16 mode.

Prints one JSON object with, for fp32 gradients and for bf16 gradients (M2FNet.set_grad_bf16):
  * "step_ms": the whole step - train_step + optimizer.step() - in three variants alternated in one process on the same model, timed
    with device events: "off" (ema_decay None), "on" (the average kept by the optimizer's kernel) and "bolt_on" (ema_decay None, then
    one torch.Tensor.lerp_ of a second flat buffer towards the flat parameter buffer: what a user had to do from outside; the buffer is
    only read, so the bf16 parameter shadows stay fresh - the cheapest bolt-on there is).  Median and min over --reps rounds and the
    medians' differences;
  * "alone": the optimizer's kernel alone with and without the average, --burst back-to-back launches per timed interval so that the
    event pair's own overhead is amortised, with the bytes each moves per parameter (p, m, v read and written, g read, the two bf16
    shadows written: 28 + 4 B besides g; the average read and written: + 8 B) and the achieved TB/s; and the lerp_ alone (12 B);
  * "exchange_us": one averaged_parameters() entry plus exit (two exchange launches, 16 B per parameter each), nothing inside.
--kernel-stats MODE (off | on | bolt_on) [--gradients fp32 | bf16]: only runs --reps whole steps in that mode, for a separate run
  under rocprofv3 --kernel-trace --stats; prints nothing else.
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

MODES = ("off", "on", "bolt_on")
DECAY = 0.999


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--kernel-stats", choices=MODES, default=None)
    ap.add_argument("--gradients", choices=["fp32", "bf16"], default=None, help="only this gradient precision (default: both)")
    args = ap.parse_args()
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    eng = model.engine()
    n_params = sum(n for (_, _, n, _) in eng.items)
    flat = eng.flat                                              # read only below: the shadows stay fresh
    second = torch.zeros_like(flat)                              # the bolt-on's average

    def step(mode):
        opt.ema_decay = DECAY if mode == "on" else None
        model.train_step(*batch)
        opt.step()
        if mode == "bolt_on":
            second.lerp_(flat, 1.0 - DECAY)

    out = {"workload": wl["name"], "precision": "bf16", "parameters": n_params, "flat_elements": flat.numel(), "decay": DECAY}
    for grads in ("fp32", "bf16"):
        if args.gradients and grads != args.gradients:
            continue
        assert model.set_grad_bf16(grads == "bf16") == (grads == "bf16")
        for mode in MODES:                                       # plans, graphs, the average buffer: warm every mode
            for _ in range(3):
                step(mode)
        torch.cuda.synchronize()
        assert eng.shadows_fresh()
        if args.kernel_stats:
            for _ in range(args.reps):
                step(args.kernel_stats)
            torch.cuda.synchronize()
            continue
        times = {m: [] for m in MODES}
        for _ in range(args.reps):
            for mode in MODES:
                times[mode].append(timed(lambda: step(mode)))
        med = {m: statistics.median(v) for m, v in times.items()}
        res = {"step_ms": {m: {"median": med[m], "min": min(times[m])} for m in MODES}, "rounds": args.reps}
        res["step_ms"]["on_minus_off_median"] = med["on"] - med["off"]
        res["step_ms"]["bolt_on_minus_off_median"] = med["bolt_on"] - med["off"]
        res["step_ms"]["on_minus_bolt_on_median"] = med["on"] - med["bolt_on"]
        # the launches alone, on the gradients of the last step
        gbytes = 2 if grads == "bf16" else 4

        def adam_burst(decay):
            opt.ema_decay = decay
            for _ in range(args.burst):
                opt.step()

        def lerp_burst():
            for _ in range(args.burst):
                second.lerp_(flat, 1.0 - DECAY)
        alone = {}
        for name, fn, per_param in (("adam_off", lambda: adam_burst(None), 28 + gbytes), ("adam_on", lambda: adam_burst(DECAY), 36 + gbytes),
                                    ("lerp", lerp_burst, 12)):
            fn()
            torch.cuda.synchronize()
            ts = [timed(fn) / args.burst for _ in range(max(5, args.reps // 4))]
            us = statistics.median(ts) * 1e3
            alone[name] = {"us_median": us, "us_min": min(ts) * 1e3, "bytes_per_parameter": per_param,
                           "TB_per_s": n_params * per_param / (us * 1e-6) / 1e12}
        alone["on_over_off_TB_per_s"] = alone["adam_on"]["TB_per_s"] / alone["adam_off"]["TB_per_s"]
        res["alone"] = alone

        def round_trip():
            with opt.averaged_parameters():
                pass
        round_trip()
        torch.cuda.synchronize()
        ts = [timed(round_trip) for _ in range(max(5, args.reps // 4))]
        res["exchange_us"] = {"entry_plus_exit_median": statistics.median(ts) * 1e3, "min": min(ts) * 1e3, "bytes_per_parameter": 32}
        opt.ema_decay = None
        out[grads + "_gradients"] = res
    if not args.kernel_stats:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
