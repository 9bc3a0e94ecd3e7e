"""Snapshot and restore of live dialogues (DialogueStream.snapshot / restore, csrc/stream_cache.hip), at C3 width.

A causal stream (capacity 512) of S slots, dense or paged (page_rows 16, just enough pages), every slot holding a history of n
utterances loaded by a chunked prefill.  Per cell, --rounds alternated rounds of
    copy    - torch's device-to-device copy_ of a tensor of the snapshot's byte count: the yardstick
    gather  - the gather launch alone (runtime.StreamPlan.gather: caches -> packed), per-entry arrays already on the device
    scatter - the scatter launch alone (packed -> caches)
    restore - DialogueStream.restore(snap) as a caller sees it: validation, pages, uploads, launch
    prefill - reset() and prefill of the same history: what a stream without snapshots pays to get the dialogues back
each --steps calls (prefill: one) between one hipEvent pair; median and range over the rounds, us per call, and the payload rate
(snapshot bytes per second: every byte is read once and written once).  One JSON line per cell.
    python tools/bench_stream_snapshot.py --precisions bf16,fp32 --history 16,64,512"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
from bench_streaming import config, timed  # noqa: E402


def stats(xs, digits=1):
    return {"median": round(float(np.median(xs)), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def cell(args, model, precision, S, n, form):
    cfg = model.m2f_config
    gen = torch.Generator().manual_seed(1)
    R = args.page_rows
    text = (torch.randn(S, n, cfg.d_text, generator=gen) * 0.6).cuda()
    audio = (torch.randn(S, n, cfg.d_audio, generator=gen) * 0.2).cuda()
    with torch.inference_mode():
        st = model.stream(S, max_chunk=args.chunk) if form == "dense" else model.stream(S, max_chunk=args.chunk, pages=S * -(-n // R), page_rows=R)

        def prefill():
            st.reset()
            st.prefill(text, audio)
        prefill()
        snap = st.snapshot()
        assert snap.lengths == [n] * S
        other = torch.empty_like(snap.data)
        packed = torch.empty_like(snap.data)
        dev = snap.data.device
        slots = torch.arange(S, dtype=torch.int32, device=dev)
        lengths = torch.tensor(snap.lengths, dtype=torch.int32, device=dev)
        offsets = torch.tensor(snap.row_offsets, dtype=torch.int64, device=dev)
        calls = {"copy": (lambda: other.copy_(snap.data), args.steps),
                 "gather": (lambda: st.plan.gather(slots, lengths, offsets, packed), args.steps),
                 "scatter": (lambda: st.plan.scatter(slots, lengths, offsets, snap.data), args.steps),
                 "restore": (lambda: st.restore(snap), args.steps),
                 "prefill": (prefill, 1)}
        for _ in range(args.warmup):
            for fn, _k in calls.values():
                fn()
        torch.cuda.synchronize()
        assert torch.equal(packed.view(torch.int16), snap.data.view(torch.int16)), "gather after scatter must return the snapshot"
        times = {k: [] for k in calls}
        for _ in range(args.rounds):                                               # alternated: drift lands on every call alike
            for k, (fn, steps) in calls.items():
                times[k].append(timed(fn, steps))
        row = {"precision": precision, "S": S, "history": n, "form": form, "page_rows": R if form == "paged" else None,
               "snapshot_bytes": snap.nbytes, "rounds": args.rounds, "steps_per_round": args.steps}
        for k, v in times.items():
            row[k + "_us"] = stats(v)
        for k in ("copy", "gather", "scatter"):
            row[k + "_GBps"] = round(snap.nbytes / (row[k + "_us"]["median"] * 1e-6) / 1e9, 1)
        row["gather_over_copy"] = round(row["copy_us"]["median"] / row["gather_us"]["median"], 2)
        row["scatter_over_copy"] = round(row["copy_us"]["median"] / row["scatter_us"]["median"], 2)
        row["prefill_over_restore"] = round(row["prefill_us"]["median"] / row["restore_us"]["median"], 1)
        print(json.dumps(row), flush=True)
        st.close()
    del snap, other, packed
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp32")
    ap.add_argument("--streams", default="64")
    ap.add_argument("--history", default="16,64,512")
    ap.add_argument("--forms", default="dense,paged")
    ap.add_argument("--page-rows", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    for precision in args.precisions.split(","):
        torch.manual_seed(0)
        model = M2FNet(config("c3"), precision=precision, context=(None, 0)).cuda().eval()
        for S in (int(x) for x in args.streams.split(",")):
            for n in (int(x) for x in args.history.split(",")):
                for form in args.forms.split(","):
                    cell(args, model, precision, S, n, form)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
