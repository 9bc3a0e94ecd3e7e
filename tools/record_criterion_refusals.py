"""Record what the step entry points answer to every combination of their criterion arguments into tests/golden/criterion_refusals.json.
tests/test_criterion_resolve_cpu.py replays every case with the functions of this file and requires the same outcome, word for word.
The fixture is recorded ONCE, on the commit before the per-criterion argument checkers became one rule table (criterion.resolve); a run
that differs from it is a finding about the table, not a reason to record again.

A CPU ``M2FNet`` of the small synthetic config (no device needed: every refusal is raised before the engine is asked for, and a call
that passes the checks fails with the engine's "runs only on an MI355X" error - recorded as "reached the engine") is driven through
``M2FNet.train_step``, ``M2FNet.eval_step`` and ``Distiller.train_step`` with
    every subset of teacher_logits, distill, focal_gamma, crf, rdrop, supcon, aux (valid values),
    each subset with crf: class_weights given or not x label_smoothing 0.0 or 0.1 x a trainable or a frozen block,
    each subset with aux: a trainable or a frozen head.
Stored: the distinct outcomes once ("messages": "<exception type>: <message>" or "reached the engine") and, per case, its index.

    python tools/record_criterion_refusals.py [--out FILE]           (no GPU; writes the fixture)"""
import argparse
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
FIXTURE = os.path.join(ROOT, "tests", "golden", "criterion_refusals.json")
ARGS = ("teacher_logits", "distill", "focal_gamma", "crf", "rdrop", "supcon", "aux")
ENTRIES = ("train_step", "eval_step", "distiller")
B, L, AUX_CLASSES = 2, 5, 3
ENGINE = "reached the engine"


def cases():
    """-> [(entry, subset, class_weights given, label_smoothing or None, crf trainable, aux trainable)], in the fixture's order"""
    out = []
    for entry in ENTRIES:
        for n in range(len(ARGS) + 1):
            for subset in itertools.combinations(ARGS, n):
                crf_axes = list(itertools.product((False, True), (0.0, 0.1), (True, False))) if "crf" in subset else [(False, None, True)]
                for (cw, ls, crf_t), aux_t in itertools.product(crf_axes, (True, False) if "aux" in subset else (True,)):
                    out.append((entry, subset, cw, ls, crf_t, aux_t))
    return out


def key(case):
    entry, subset, cw, ls, crf_t, aux_t = case
    return "%s|%s|cw=%d,ls=%s,crf_trainable=%d,aux_trainable=%d" % (entry, ",".join(subset), cw, ls, crf_t, aux_t)


class Rig:
    """The CPU model, a Distiller over it, one batch and one valid value per criterion argument"""

    def __init__(self):
        import synth
        import mer_amd  # noqa: F401
        from mer_amd.aux_head import AuxiliaryHead
        from mer_amd.crf import LinearChainCRF
        from mer_amd.distill import Distiller
        from mer_amd.model import M2FNet
        cfg = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1)
        torch.manual_seed(0)
        self.model = M2FNet(cfg)
        self.distiller = Distiller(self.model, M2FNet(cfg), alpha=0.5, temperature=2.0)
        self.batch = synth.make_inputs(cfg, B, L, None, "randn", seed=1)
        C, hidden = self.model.m2f_config.cls_out, self.model.m2f_config.cls_hidden
        self.class_weights = torch.ones(C)
        self.crf = {t: LinearChainCRF(C) for t in (True, False)}
        self.crf[False].params.requires_grad_(False)
        self.head = {t: AuxiliaryHead(hidden, AUX_CLASSES) for t in (True, False)}
        self.head[False].params.requires_grad_(False)
        self.values = {"teacher_logits": torch.zeros(B, L, C), "distill": (0.5, 2.0), "focal_gamma": 2.0, "rdrop": 1.0,
                       "supcon": (0.1, 0.1)}
        self.aux_labels = torch.randint(0, AUX_CLASSES, (B, L), generator=torch.Generator().manual_seed(2))

    def outcome(self, case) -> str:
        from mer_amd.runtime import HipError
        entry, subset, cw, ls, crf_t, aux_t = case
        kw = {name: self.values[name] for name in subset if name in self.values}
        if "crf" in subset:
            kw["crf"] = self.crf[crf_t]
        if "aux" in subset:
            kw["aux"] = (self.head[aux_t], self.aux_labels, 0.5)
        if cw:
            kw["class_weights"] = self.class_weights
        if ls is not None:
            kw["label_smoothing"] = ls
        try:
            if entry == "train_step":
                self.model.train_step(*self.batch, **kw)
            elif entry == "eval_step":
                self.model.eval_step(*self.batch, None, **kw)
            else:
                self.distiller.train_step(*self.batch, **kw)
        except HipError as e:
            if str(e).startswith("M2FNet runs only on an MI355X"):
                return ENGINE
            return "HipError: %s" % e
        except Exception as e:                              # noqa: BLE001 (the outcome IS the exception)
            return "%s: %s" % (type(e).__name__, e)
        return "returned"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    rig, messages, index = Rig(), [], {}
    for case in cases():
        got = rig.outcome(case)
        if got not in messages:
            messages.append(got)
        index[key(case)] = messages.index(got)
    with open(args.out, "w") as f:
        json.dump({"messages": messages, "cases": index}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", len(index), "cases,", len(messages), "distinct outcomes")
    for i, m in enumerate(messages):
        print("%4d x %s" % (sum(1 for v in index.values() if v == i), m))


if __name__ == "__main__":
    main()
