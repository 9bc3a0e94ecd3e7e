"""What speaker-aware attention heads cost (M2FNet(speaker_heads=(2, 2))): off (the kernels that always ran) against (2, 2) (the SPK
instantiations: two same-speaker and two other-speaker heads at every site), alternated, on
  c3      BASELINE C3 (roberta-large 1024 + wav2vec2 768, 64 dialogues x 16 utterances, bf16): an eval forward and a train step - the
          short dialogue kernel (attention.hip);
  long    the long-dialogue set of tools/long_dialogue_step.py (16 dialogues of 8..110 utterances, packed plan): a train step - the
          long-dialogue forward (attention_dlong.hip);
  stream  a stream step at C3 width, S = 64 live dialogues with a history of 16 and of 512 utterances, dense and paged caches
          (attention_stream.hip; the cells of tools/bench_stream_paged.py).
Speakers: three per dialogue in turns of two utterances.  Every model / stream is built and warmed (graph captured) first; then --rounds
rounds of [off, on], each --steps replayed calls between one hipEvent pair; the reported time of a form is the median over the rounds,
with its range.  One JSON line per cell.
    python tools/bench_speaker_heads.py --workloads c3,long,stream --rounds 7 --steps 20"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
import long_dialogue_step as lds  # noqa: E402
from bench_context_window import c3_config, full_batch  # noqa: E402
from bench_position_bias import alternate, stats  # noqa: E402
from bench_stream_paged import at_history  # noqa: E402

FORMS = {"off": None, "on": (2, 2)}


def speaker_ids(B, L):
    """uint8 [B, L] on the device: three speakers per dialogue in turns of two utterances"""
    return (((torch.arange(L)[None, :] // 2) + torch.arange(B)[:, None]) % 3).to(torch.uint8).cuda()


def steps_cell(args, name, cfg, batch, context, forward):
    ids = speaker_ids(*batch[2].shape)
    models = {}
    for f, heads in FORMS.items():
        torch.manual_seed(0)
        models[f] = M2FNet(cfg, precision=args.precision, context=context, speaker_heads=heads).cuda()
    kw = {f: ({} if FORMS[f] is None else {"speakers": ids}) for f in FORMS}
    calls = {}
    for f, m in models.items():
        if forward:
            def fwd(m=m, f=f):
                m.eval()
                with torch.inference_mode():
                    m(*batch[:3], **kw[f])
            calls[f + "_forward_us"] = fwd
    times = alternate(calls, args.rounds, args.steps, args.warmup) if calls else {}
    calls = {f + "_train_step_us": (lambda m=m, f=f: m.train().train_step(*batch, use_graph=True, **kw[f])) for f, m in models.items()}
    times.update(alternate(calls, args.rounds, args.steps, args.warmup))
    pl = next(iter(models["on"].engine().plans.values()))
    assert pl.speakers == FORMS["on"] and all(p.speakers is None for p in models["off"].engine().plans.values())
    row = {"workload": name, "precision": args.precision, "context": context, "speaker_heads": FORMS["on"],
           "plan": {"B": pl.B, "L": pl.L, "T": pl.T, "packed": bool(pl.packed)}, "rounds": args.rounds, "steps_per_round": args.steps}
    row.update({k: stats(v) for k, v in times.items()})
    print(json.dumps(row), flush=True)
    del models
    torch.cuda.empty_cache()


def stream_cells(args):
    S, R = 64, 16
    gen = torch.Generator().manual_seed(1)
    models = {}
    for f, heads in FORMS.items():
        torch.manual_seed(0)
        models[f] = M2FNet(c3_config(), precision=args.precision, context=(None, 0), speaker_heads=heads).cuda().eval()
    cfg = models["off"].m2f_config
    text = (torch.randn(S, cfg.d_text, generator=gen) * 0.6).cuda()
    audio = (torch.randn(S, cfg.d_audio, generator=gen) * 0.2).cuda()
    new_ids = torch.ones(S, dtype=torch.uint8).cuda()
    for n in (int(x) for x in args.history.split(",")):
        with torch.inference_mode():
            sts = {(f, c): at_history(models[f], S, n, 1, S * -(-n // R) if c == "paged" else None, R) for f in FORMS for c in ("dense", "paged")}
            assert all(st.speaker_heads == FORMS[f] for (f, _), st in sts.items())
            for (f, _), st in sts.items():
                if st.speaker_cache is not None:              # (the history's ids: three speakers in turns of two)
                    st.speaker_cache.copy_(speaker_ids(S, st.capacity))
            calls = {f"{f}_{c}_step_us": (lambda st=st, f=f: st.step(text, audio, **({} if FORMS[f] is None else {"speakers": new_ids})))
                     for (f, c), st in sts.items()}
            times = alternate(calls, args.rounds, args.steps, args.warmup)
        row = {"workload": "stream", "precision": args.precision, "S": S, "n": n, "page_rows": R, "speaker_heads": FORMS["on"],
               "rounds": args.rounds, "steps_per_round": args.steps}
        row.update({k: stats(v) for k, v in times.items()})
        print(json.dumps(row), flush=True)
        for st in sts.values():
            st.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,long,stream")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--history", default="16,512")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    for name in args.workloads.split(","):
        if name == "c3":
            steps_cell(args, name, c3_config(), full_batch(64, 16, 1024, 768), (None, 0), forward=True)
        elif name == "long":
            steps_cell(args, name, lds.config(), lds.batch()[0], (None, 0), forward=False)
        elif name == "stream":
            stream_cells(args)
        else:
            raise SystemExit(f"unknown workload {name!r} (c3, long, stream)")


if __name__ == "__main__":
    main()
