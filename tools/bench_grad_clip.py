"""Gradient clipping by global norm (FusedAdam(max_grad_norm=...), csrc/gradnorm.hip) at bench geometry C3, bf16 mode.

Prints one JSON object with, for fp32 gradients and for bf16 gradients (M2FNet.set_grad_bf16):
  * "step_ms": the whole step - train_step + optimizer.step() - with clipping off, on with plain loads and on with nontemporal loads
    in the sum-of-squares kernel, the three alternated in one process on the same model, timed with device events: median and min
    over --reps rounds, and the medians' differences to "off";
  * "alone": the two norm launches alone and the optimizer's kernel alone (clipping off), --burst back-to-back launches per timed
    interval so that the event pair's own overhead is amortised, with the bytes each reads / writes and the achieved GB/s.  Back to
    back the gradients may be served from the Infinity Cache (the bf16 buffer fits in it): the in-step figures above and a
    --kernel-stats run are the ones that describe a training step.
--kernel-stats MODE (off | plain | nontemporal) [--gradients fp32 | bf16]: only runs --reps whole steps in that mode, for a separate
  run under rocprofv3 --kernel-trace --stats (the norm kernels' and the Adam kernel's own time inside the step); prints nothing else.
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

MODES = ("off", "plain", "nontemporal")
MAX_NORM = 1.0


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

    def set_mode(mode):
        opt.max_grad_norm = None if mode == "off" else MAX_NORM
        runtime.GRAD_NORM_NONTEMPORAL = mode == "nontemporal"

    def step():
        model.train_step(*batch)
        opt.step()

    out = {"workload": wl["name"], "precision": "bf16", "parameters": n_params, "max_grad_norm": MAX_NORM}
    for grads in ("fp32", "bf16"):
        if args.gradients and grads != args.gradients:
            continue
        assert model.set_grad_bf16(grads == "bf16") == (grads == "bf16")
        for mode in MODES:                                       # plans, graphs, scratch: warm every mode
            set_mode(mode)
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        if args.kernel_stats:
            set_mode(args.kernel_stats)
            for _ in range(args.reps):
                step()
            torch.cuda.synchronize()
            continue
        times = {m: [] for m in MODES}
        for _ in range(args.reps):
            for mode in MODES:
                set_mode(mode)
                times[mode].append(timed(step))
        med = {m: statistics.median(v) for m, v in times.items()}
        res = {"step_ms": {m: {"median": med[m], "min": min(times[m])} for m in MODES}, "rounds": args.reps}
        res["step_ms"]["plain_minus_off_median"] = med["plain"] - med["off"]
        res["step_ms"]["nontemporal_minus_off_median"] = med["nontemporal"] - med["off"]
        # the launches alone, on the gradients of the last step
        set_mode("off")
        gbuf = eng.grad_bf16_buf if eng.grad_bf16_buf is not None else eng.ensure_grad()
        gbytes = n_params * gbuf.element_size()
        scratch = runtime.grad_norm_scratch(eng.cfg, dev)
        record = torch.zeros(4, dtype=torch.float32, device=dev)

        def norm_burst(nt):
            for _ in range(args.burst):
                runtime.grad_sumsq(eng.cfg, gbuf, scratch, nontemporal=nt)
                runtime.grad_norm_finalize(eng.cfg, scratch, record, MAX_NORM, None)

        def adam_burst():
            for _ in range(args.burst):
                opt.step()
        alone = {}
        for name, fn, nbytes in (("norm_plain", lambda: norm_burst(False), gbytes), ("norm_nontemporal", lambda: norm_burst(True), gbytes),
                                 # p, m, v read and written, g read, the two bf16 shadows written: 24 + 4 B per parameter besides g
                                 ("adam", adam_burst, n_params * 28 + gbytes)):
            fn()
            torch.cuda.synchronize()
            ts = [timed(fn) / args.burst for _ in range(max(5, args.reps // 4))]
            us = statistics.median(ts) * 1e3
            alone[name] = {"us_median": us, "us_min": min(ts) * 1e3, "bytes": nbytes, "GB_per_s": nbytes / (us * 1e-6) / 1e9}
        res["alone"] = alone
        res["record"] = [float(x) for x in record.cpu()]
        out[grads + "_gradients"] = res
    if not args.kernel_stats:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
