"""The model watch (FusedAdam(watch=ModelWatch(...)), csrc/tensor_stats.hip) at bench geometry C3, bf16 mode.

Prints one JSON object with
  * "step_ms": the whole step - train_step + optimizer.step() - without a watch against a watch with log_freq=1 (EVERY step due: the
    cost of a due step; at log_freq=100 a hundredth of it per step), alternated pair by pair in one process on the same model, timed
    with device events after warm-up: the medians and the median of the per-pair differences over --pairs pairs, for log="all", for
    log="all" with bf16 gradients (M2FNet.set_grad_bf16) and for log=[gradients, parameters, updates];
  * "alone": over the gradient buffer of the last step (fp32, then bf16) and over a constant buffer (the histogram's worst case: every
    value in one bin), pass 1 (+ its finalize launch) alone and pass 2 alone, beside gradnorm.hip's sum-of-squares pass (+ its
    finalize launch) on the same buffer in the same run: --burst back-to-back launches per timed interval, the bytes each reads and
    the achieved GB/s.  Back to back, a buffer below the Infinity Cache's 256 MiB (the bf16 one) may be served from it.
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
from mer_amd.watch import ModelWatch  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402

CASES = (("all_fp32_gradients", "all", False), ("all_bf16_gradients", "all", True),
         ("gradients_parameters_updates", ["gradients", "parameters", "updates"], False))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--bins", type=int, default=64)
    args = ap.parse_args()
    if args.pairs < 30:
        ap.error("--pairs must be at least 30")
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).train()
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
    eng = model.engine()
    n_params = sum(n for (_, _, n, _) in eng.items)

    def step():
        model.train_step(*batch)
        opt.step()

    out = {"workload": wl["name"], "precision": "bf16", "parameters": n_params, "bins": args.bins, "pairs": args.pairs, "step_ms": {}}
    for name, log, g16 in CASES:
        assert model.set_grad_bf16(g16) == g16
        watch = ModelWatch(model, log=log, log_freq=1, bins=args.bins)
        for w in (None, watch, None, watch):                     # plans, graphs, record buffers: warm both forms
            opt.watch = w
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        off, on = [], []
        for _ in range(args.pairs):
            opt.watch = None
            off.append(timed(step))
            opt.watch = watch
            on.append(timed(step))
        opt.watch = None
        rec = watch.read()
        out["step_ms"][name] = {"off_median": statistics.median(off), "on_median": statistics.median(on),
                                "pair_difference_median": statistics.median(b - a for a, b in zip(off, on)),
                                "off_min": min(off), "on_min": min(on), "kinds": list(watch.kinds), "last_step": rec["step"]}

    # the passes alone
    scratch_n = runtime.grad_norm_scratch(eng.cfg, dev)
    record_n = torch.zeros(4, dtype=torch.float32, device=dev)
    scratch, record = runtime.tensor_stats_buffers(eng.cfg, args.bins, dev)
    out["alone"] = {}
    model.set_grad_bf16(False)
    step()
    buffers = [("fp32_gradients", eng.ensure_grad())]
    assert model.set_grad_bf16(True)
    step()
    buffers.append(("bf16_gradients", eng.grad_bf16_buf))
    buffers.append(("fp32_constant", torch.full_like(eng.ensure_grad(), 0.5)))
    torch.cuda.synchronize()
    for bname, buf in buffers:
        nbytes = n_params * buf.element_size()
        runtime.tensor_stats(eng.cfg, buf, scratch, record, args.bins)      # the rows pass 2 alone reads

        def burst(fn):
            def run():
                for _ in range(args.burst):
                    fn()
            return run

        def norm():
            runtime.grad_sumsq(eng.cfg, buf, scratch_n)
            runtime.grad_norm_finalize(eng.cfg, scratch_n, record_n, 1.0, None)
        forms = (("gradnorm_sumsq", norm),
                 ("pass1_statistics", lambda: runtime.tensor_stats(eng.cfg, buf, scratch, record, args.bins, passes=1)),
                 ("pass2_histogram", lambda: runtime.tensor_stats(eng.cfg, buf, scratch, record, args.bins, passes=2)))
        res = {}
        samples = {k: [] for k, _ in forms}
        for k, fn in forms:
            burst(fn)()
        torch.cuda.synchronize()
        for _ in range(max(8, args.pairs // 4)):                   # alternated, so that the three share whatever else the machine does
            for k, fn in forms:
                samples[k].append(timed(burst(fn)) / args.burst)
        for k, _ in forms:
            us = statistics.median(samples[k]) * 1e3
            res[k] = {"us_median": us, "us_min": min(samples[k]) * 1e3, "bytes": nbytes, "GB_per_s": nbytes / (us * 1e-6) / 1e9}
        res["pass1_over_gradnorm_rate"] = res["pass1_statistics"]["GB_per_s"] / res["gradnorm_sumsq"]["GB_per_s"]
        out["alone"][bname] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
