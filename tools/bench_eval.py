"""One validation pass with the host rule against the device rule (runtime.device_metrics, M2FNet.eval_step, csrc/metrics.hip).

Both rules are src/train.py::validate itself, with `model.device_metrics` off (eager forward, the criterion + .item(),
argmax + two mask gathers + two .cpu() copies, sklearn on the host) and on (one replayed graph per batch, one read after the last
batch), on the same model and the same seeded batches in ONE process, alternated: --rounds passes of each after --warmup passes of
each, timed with the host clock around a pass that ends in a device synchronise (the host rule waits for the device in every batch
anyway).  Prints one JSON object: per workload and precision the per-batch time (pass time / batches) of both rules - median, min,
max over the rounds -, their ratio, and the three numbers both rules returned (they must agree: 1e-12 / 2e-5).

Workloads: "meld" = the shipped geometry (768 / 768 / 768, 6 + 5 layers) on MELD-like ragged batches, 32 dialogues of 1 .. 33
utterances (three L-buckets and a smaller last batch); "c3" = BASELINE C3 (roberta-large 1024 + wav2vec2 768), 64 dialogues x 16.
--kernel-stats: only runs --rounds device-rule passes (after warm-up), for a separate run under rocprofv3 --kernel-trace --stats
(the two scoring kernels' own times); prints nothing.
There is no CPU path: without an MI355X the first device call raises."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import M2FCrossEntropyLoss  # noqa: E402
from bench import WORKLOADS  # noqa: E402


def batches_of(cfg, B, n_batches, max_len, ragged, seed):
    """Collated batches as the DataLoader hands them over (host tensors): text = 0.63 randn, audio = 0.23 randn, labels randint(0, 7)
    (bench.synthetic_batch's statistics); ragged: dialogue lengths uniform in 1 .. max_len, padded to the batch's longest, the last
    batch with fewer dialogues."""
    g = torch.Generator().manual_seed(seed)
    d_t, d_a = cfg["TEXT"]["embedding_size"], cfg["AUDIO"]["embedding_size"]
    out = []
    for i in range(n_batches):
        b = B if (not ragged or i < n_batches - 1) else max(B // 2 - 3, 1)
        lens = torch.randint(1, max_len + 1, (b,), generator=g) if ragged else torch.full((b,), max_len)
        L = int(lens.max())
        mask = torch.arange(L)[None, :] >= lens[:, None]
        text = torch.randn(b, L, d_t, generator=g) * 0.63
        audio = torch.randn(b, L, d_a, generator=g) * 0.23
        emotion = torch.randint(0, 7, (b, L), generator=g)
        text[mask] = 0.0
        audio[mask] = 0.0
        emotion[mask] = -1
        out.append({"text": text, "audio": audio, "emotion": emotion, "padding_mask": mask})
    return out


CASES = {
    "meld": dict(workload="c2p", B=32, n_batches=12, max_len=33, ragged=True),
    "c3": dict(workload="c3", B=64, n_batches=8, max_len=16, ragged=False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="meld,c3")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--kernel-stats", action="store_true")
    args = ap.parse_args()
    if args.rounds < 1 or args.warmup < 1:
        ap.error("--rounds and --warmup must be at least 1")
    runtime.require_gpu()                                  # (raises without an MI355X: nothing below has a host form)
    import train as tr
    tr.tqdm = lambda it, **_: it                           # no progress bars inside the timed passes
    dev = torch.device("cuda:0")
    crit = M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    out = {"rounds": args.rounds, "warmup": args.warmup, "results": []}
    for case in args.cases.split(","):
        c = CASES[case]
        wl = WORKLOADS[c["workload"]]
        batches = batches_of(wl["cfg"], c["B"], c["n_batches"], c["max_len"], c["ragged"], seed=4321)
        for dtype in args.dtypes.split(","):
            torch.manual_seed(0)
            model = M2FNet(wl["cfg"], precision=dtype).to(dev).eval()

            def one_pass(on):
                model.device_metrics = on
                t0 = time.perf_counter()
                res = tr.validate(model, batches, crit, dev)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, res

            for _ in range(args.warmup):                   # plans, graphs, scratch: both rules
                one_pass(False)
                one_pass(True)
            if args.kernel_stats:
                for _ in range(args.rounds):
                    one_pass(True)
                continue
            times, last = {False: [], True: []}, {}
            for _ in range(args.rounds):
                for on in (False, True):
                    ms, last[on] = one_pass(on)
                    times[on].append(ms / len(batches))
            row = {"case": case, "workload": wl["name"], "dtype": dtype, "batches": len(batches),
                   "rows_scored": sum(int((b["emotion"] != -1).sum()) for b in batches)}
            for on, name in ((False, "host_rule"), (True, "device_rule")):
                row[name] = {"ms_per_batch_median": statistics.median(times[on]), "ms_per_batch_min": min(times[on]),
                             "ms_per_batch_max": max(times[on]), "loss_acc_f1": list(last[on])}
            row["device_over_host_median"] = row["device_rule"]["ms_per_batch_median"] / row["host_rule"]["ms_per_batch_median"]
            out["results"].append(row)
            del model
            torch.cuda.empty_cache()
    if not args.kernel_stats:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
