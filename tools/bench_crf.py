"""The linear-chain CRF criterion (M2FNet.train_step(crf=) / eval_step(crf=) / stream(crf=); csrc/crf.hip) at bench geometry C3, bf16
mode, 64 dialogues x 16 utterances, and on the long-dialogue batch of tools/long_dialogue_step.py (16 dialogues of 8 .. 110 utterances).

Prints one JSON object.  Every figure is the median (and min) over --reps rounds (at least 5) of modes ALTERNATED in one process and
timed with device events; every mode has its own model, so no switch of criterion re-captures inside a timed step:
  * "train_ms" / "long_train_ms": train_step + optimizer.step() with the plain criterion ("ce", label_smoothing 0), with a frozen CRF
    ("crf_frozen": one launch in the criterion's place) and a trainable one ("crf_trainable": one more small reduce launch);
  * "eval_ms": eval_step with the plain criterion and with crf= (the CRF loss, the Viterbi launch, the prediction form of the rows launch);
  * "stream_ms": one stream step at S = 64 (causal context, window 16) without and with the filter launch."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import mer_amd  # noqa: E402,F401
from mer_amd.crf import LinearChainCRF  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam  # noqa: E402
from bench import WORKLOADS, synthetic_batch  # noqa: E402
import long_dialogue_step  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(steps, reps, warm=6):
    for _ in range(warm):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    times = {m: [] for m in steps}
    for _ in range(reps):
        for m, fn in steps.items():
            fn()
            times[m].append(timed(fn))
    return {m: {"median": statistics.median(v), "min": min(v)} for m, v in times.items()}


def crf_module(dev, trainable, seed=0):
    g = torch.Generator().manual_seed(seed)
    crf = LinearChainCRF(7).to(dev)
    with torch.no_grad():
        crf.params.copy_(torch.randn(crf.params.numel(), generator=g) * 0.5)
    crf.params.requires_grad_(trainable)
    return crf


def train_modes(cfg, batch, dev):
    steps = {}
    for mode in ("ce", "crf_frozen", "crf_trainable"):
        torch.manual_seed(0)
        model = M2FNet(cfg, precision="bf16").to(dev).train()
        opt = FusedAdam(model, lr=1e-4, weight_decay=0.01)
        crf = None if mode == "ce" else crf_module(dev, mode == "crf_trainable")
        copt = torch.optim.Adam(crf.parameters(), lr=1e-2) if mode == "crf_trainable" else None

        def step(model=model, opt=opt, crf=crf, copt=copt):
            model.train_step(*batch, label_smoothing=0.0, crf=crf)
            opt.step()
            if copt is not None:
                copt.step()
        steps[mode] = step
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    reps = max(args.reps, 5)
    wl = WORKLOADS["c3"]
    dev = torch.device("cuda:0")
    batch = synthetic_batch(wl["cfg"], wl["B"], wl["L"], 0, dev)
    out = {"workload": wl["name"], "precision": "bf16", "B": wl["B"], "L": wl["L"], "rounds": reps}
    out["train_ms"] = alternate(train_modes(wl["cfg"], batch, dev), reps)

    long_batch, lens = long_dialogue_step.batch(device=dev)
    out["long_train_ms"] = alternate(train_modes(long_dialogue_step.config(), long_batch, dev), reps)
    out["long_lengths"] = [int(lens.min()), int(lens.max())]

    torch.manual_seed(0)
    model = M2FNet(wl["cfg"], precision="bf16").to(dev).eval()
    frozen = crf_module(dev, False)
    scores = {m: DeviceScores(7, dev) for m in ("ce", "crf")}
    other = M2FNet(wl["cfg"], precision="bf16").to(dev).eval()
    out["eval_ms"] = alternate({"ce": lambda: model.eval_step(*batch, scores["ce"], label_smoothing=0.0),
                                "crf": lambda: other.eval_step(*batch, scores["crf"], label_smoothing=0.0, crf=frozen)}, reps)

    S = 64
    causal = M2FNet(wl["cfg"], precision="bf16", context=(16, 0)).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    text = (torch.randn(S, wl["cfg"]["TEXT"]["embedding_size"], generator=g) * 0.63).to(dev)
    audio = (torch.randn(S, wl["cfg"]["AUDIO"]["embedding_size"], generator=g) * 0.23).to(dev)
    plain, filt = causal.stream(S), causal.stream(S, crf=frozen)
    out["stream_ms"] = alternate({"plain": lambda: plain.step(text, audio), "filter": lambda: filt.step(text, audio)}, reps)
    out["stream_slots"] = S
    plain.close()
    filt.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
