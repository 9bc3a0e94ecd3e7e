"""Paged against dense streaming caches (M2FNet.stream(pages=...)), at C3 width.

pair  - the same step and the same chunked prefill through a dense and a paged stream: S live dialogues, history n.  As in
        tools/bench_streaming.py a cell's streams are opened under the window (n - 1, 0) with their counts set to n - 1 - a ring of n
        rows, so every timed call reads n live rows per slot and site while the counts grow freely; the paged stream holds
        S * ceil(n / page_rows) pages.  --rounds rounds of [dense step, paged step, dense prefill, paged prefill], alternated, each
        --steps calls between one hipEvent pair; median and range over the rounds.  `--forms dense` times the dense stream alone (the
        form that exists on a commit without paged caches, for a before / after of the dense kernels).
scale - a paged causal stream (capacity 512) of S slots on a pool of --pages pages, serving MELD-length dialogues: every slot holds
        a dialogue of clamp(round(N(9.6, 5)), 1, 33) utterances (seeded), takes one utterance per step and, when its dialogue ends, is
        reset and starts the next one.  A slot whose next row needs a page while the pool is empty waits for that step (it is left
        out of the mask).  Reported per round: ms per step - hipEvents around the whole loop, so the host's share (mask, allocator,
        table upload, resets) is in it - and utterances per second, against the pool's bytes; a dense stream of 64 slots serves the
        same traffic in the same run for comparison.
One JSON line per cell.
    python tools/bench_stream_paged.py pair --streams 64 --history 16,512
    python tools/bench_stream_paged.py scale --streams 512,2048 --pages 2048"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mer_amd  # noqa: E402,F401
from mer_amd import streaming  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from bench_streaming import config, timed  # noqa: E402


def stats(xs, digits=1):
    return {"median": round(float(np.median(xs)), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def at_history(model, S, n, T, pages, page_rows):
    """a stream whose every slot holds n - 1 utterances in a ring of n rows"""
    model.set_context(n - 1, 0)
    st = model.stream(S, max_chunk=T) if pages is None else model.stream(S, max_chunk=T, pages=pages, page_rows=page_rows)
    model.set_context(None, 0)
    if pages is not None:
        st.allocator.take(streaming.pages_needed([0] * S, [n - 1] * S, st.capacity, page_rows, True))
    st.plan.len.fill_(n - 1)
    st.lengths = [n - 1] * S
    return st


def pair(args, model, precision):
    cfg = model.m2f_config
    gen = torch.Generator().manual_seed(1)
    T, R = args.chunk, args.page_rows
    forms = args.forms.split(",")
    for S in (int(x) for x in args.streams.split(",")):
        for n in (int(x) for x in args.history.split(",")):
            text = (torch.randn(S, T, cfg.d_text, generator=gen) * 0.6).cuda()
            audio = (torch.randn(S, T, cfg.d_audio, generator=gen) * 0.2).cuda()
            new_t, new_a = text[:, 0].contiguous(), audio[:, 0].contiguous()
            with torch.inference_mode():
                sts = {f: at_history(model, S, n, T, S * -(-n // R) if f == "paged" else None, R) for f in forms}
                calls = {}
                for f, st in sts.items():
                    calls[f + "_step_us"] = lambda st=st: st.step(new_t, new_a)
                    calls[f + "_prefill_us"] = lambda st=st: st.prefill(text, audio)
                for _ in range(args.warmup):
                    for c in calls.values():
                        c()
                torch.cuda.synchronize()
                times = {k: [] for k in calls}
                for _ in range(args.rounds):                                       # alternated: drift lands on every form alike
                    for k, c in calls.items():
                        times[k].append(timed(c, args.steps if k.endswith("step_us") else args.prefill_steps))
            row = {"mode": "pair", "precision": precision, "S": S, "n": n, "chunk": T, "page_rows": R, "rounds": args.rounds,
                   "steps_per_round": args.steps}
            row.update({k: stats(v) for k, v in times.items()})
            for f, st in sts.items():
                row[f + "_cache_bytes"] = st.plan.cache_bytes()
                st.close()
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()


def serve(st, text, audio, steps, seed):
    """`steps` steps of the traffic above on `st`; -> (ms per step, utterances served, steps in which a slot had to wait)"""
    S = st.max_streams
    rng = np.random.default_rng(seed)
    draw = lambda k: np.clip(np.rint(rng.normal(9.6, 5.0, k)), 1, 33).astype(int).tolist()          # noqa: E731
    target = draw(S)
    served = waits = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        act = [True] * S
        if st.allocator is not None:
            need = streaming.pages_needed(st.lengths, [1] * S, st.capacity, st.page_rows, False)
            for s in st.allocator.shortfall(need):                              # the pool is empty: these slots wait a step
                act[s] = False
            waits += not all(act)
        st.step(text, audio, act)
        served += sum(act)
        done = [s for s in range(S) if st.lengths[s] >= target[s]]
        if done:
            st.reset(done)
            for s, n in zip(done, draw(len(done))):
                target[s] = n
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, served, waits


def scale(args, model, precision):
    cfg = model.m2f_config
    gen = torch.Generator().manual_seed(1)
    bf16 = precision == "bf16"
    cells = [(64, None)] + [(int(x), args.pages) for x in args.streams.split(",")]
    with torch.inference_mode():
        sts = []
        for S, pages in cells:
            st = model.stream(S, pages=pages, page_rows=args.page_rows)
            text = (torch.randn(S, cfg.d_text, generator=gen) * 0.6).cuda()
            audio = (torch.randn(S, cfg.d_audio, generator=gen) * 0.2).cuda()
            serve(st, text, audio, 40, 0)                                          # warm: plans, the graph, slots spread over their dialogues
            sts.append((st, text, audio, []))
        for r in range(args.rounds):                                               # alternated
            for st, text, audio, rows in sts:
                rows.append(serve(st, text, audio, args.steps, 1 + r))
    base = None
    for (S, pages), (st, _, _, rows) in zip(cells, sts):
        ms = [x[0] for x in rows]
        ups = [x[1] / (x[0] * 1e-3 * args.steps) for x in rows]
        row = {"mode": "scale", "precision": precision, "S": S, "pages": pages, "page_rows": args.page_rows if pages else None,
               "ms_per_step": stats(ms, 3), "utterances_per_s": stats(ups, 0), "cache_bytes": st.plan.cache_bytes(),
               "dense_cache_bytes_at_S": streaming.cache_bytes(cfg, S, 512, bf16=bf16), "steps_with_a_waiting_slot": sum(x[2] for x in rows),
               "rounds": args.rounds, "steps_per_round": args.steps, "launches_per_step": st.plan.num_launches()}
        if pages is None:
            base = row["utterances_per_s"]["median"]
        elif base:
            row["x_dense_64"] = round(row["utterances_per_s"]["median"] / base, 2)
        print(json.dumps(row), flush=True)
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["pair", "scale"])
    ap.add_argument("--precisions", default="bf16")
    ap.add_argument("--streams", default=None, help="pair: 64; scale: 512,2048")
    ap.add_argument("--history", default="16,512")
    ap.add_argument("--forms", default="dense,paged")
    ap.add_argument("--pages", type=int, default=2048)
    ap.add_argument("--page-rows", type=int, default=16)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prefill-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.streams is None:
        args.streams = "64" if args.mode == "pair" else "512,2048"
    for precision in args.precisions.split(","):
        torch.manual_seed(0)
        model = M2FNet(config("c3"), precision=precision, context=(None, 0)).cuda().eval()
        (pair if args.mode == "pair" else scale)(args, model, precision)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
