"""Record the bits of the optimizer kernels (csrc/adam.hip, csrc/sam.hip over csrc/param_walk.h: the flat, shadow-writing, grouped and
slice forms of the Adam update with and without the weight average, the exchange, the SAM perturbation and restore) into
tests/golden/optimizer_kernel_bits.npz.  tests/test_optimizer_kernel_bits_gpu.py replays `cases()` with the functions of this file and
holds every entry to these bits.  The suite's other optimizer tests hold the kernels to EACH OTHER's bits and to float64 inside a
tolerance; a change that moves all of them together (a contracted multiply-add in the shared element function, another fill of a
shadow's pad columns) passes those and shows here.  The fixture is recorded ONCE, on the commit before such a change (it carries that
commit's name); a run that differs from it is a finding about the kernels, not a reason to record again.

Layouts: SMALL and WIDE of tests/test_sam_kernels_gpu.py (cols % 4 != 0, rows no multiple of 64 or of 8, 1-D tensors shorter and longer
than a tile with a short last group, more than one block in every form).  Buffers are the caller's own, from
numpy.random.RandomState(seed) (the same stream in every numpy version), with a sentinel in every pad between tensors; every case runs
STEPS consecutive steps and every output buffer goes WHOLE (pads included) into a SHA-256 after each step:
    adam            m2f_adam_step / _g16 / _ema / _g16_ema                        p, m, v(, ema)
    shadowed        m2f_adam_step_shadowed_range(_ema), everything / a sub-range  p, m, v, sh(, ema)
    grouped         m2f_adam_step_grouped(_ema), with and without shadows, three groups (the second decoupled), one tensor in none
    exchange        m2f_ema_exchange once (step 1) and twice (step 2)             p, ema
    sam             m2f_grad_sumsq + m2f_sam_perturb, then m2f_sam_restore        p, saved(, sh) after the perturbation, p after the
                                                                                  restore, and the 4-float record of each step itself
each with fp32 and bf16 gradients and with grad_scale absent and set; the averaging forms with ema_w 1 and 0.1.

    python tools/record_optimizer_bits.py --commit NAME [--out FILE]           (on the GPU; writes the fixture)"""
import argparse
import ctypes
import dataclasses
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "optimizer_kernel_bits.npz")
DEV = "cuda"
STEPS = 3
SENTINEL = 12345.678
GRAD_SCALE = 3.0
EMA_WS = (None, 1.0, 0.1)
# (lr, betas, eps, weight_decay, decoupled) of the three groups; a step's rows carry the step count
GROUPS = ((1e-3, (0.9, 0.999), 1e-8, 0.01, False), (5e-4, (0.8, 0.99), 1e-6, 0.1, True), (2e-3, (0.95, 0.98), 1e-7, 0.0, False))
UNOWNED = 4                               # the tensor of no group


def layouts():
    """{name: M2FConfig}: the two layouts of tests/test_sam_kernels_gpu.py"""
    import synth
    from mer_amd import layout
    small = layout.M2FConfig.from_model_config(synth._cfg(50, 20, 36, 2, 2, 2, 1, 1, 1, hid=50, ncls=3))
    wide = dataclasses.replace(layout.M2FConfig.from_model_config(synth._cfg(24, 20, 20, 2, 2, 2, 1, 1, 1, hid=20, ncls=2)), dim_ff=4101)
    return {"small": small, "wide": wide}


def cases():
    """-> list of dicts, one stored block and one test case each; `id` is the block's key"""
    out = []
    for name in ("small", "wide"):
        for g16, gs, w in itertools.product((0, 1), (0, 1), EMA_WS):
            out.append(dict(entry="adam", layout=name, g16=g16, gs=gs, ema_w=w))
            for sub in (0, 1):
                out.append(dict(entry="shadowed", layout=name, g16=g16, gs=gs, ema_w=w, sub=sub))
                for sh in (0, 1):
                    out.append(dict(entry="grouped", layout=name, g16=g16, gs=gs, ema_w=w, sub=sub, sh=sh))
        out.append(dict(entry="exchange", layout=name))
        for g16, gs, sh in itertools.product((0, 1), (0, 1), (0, 1)):
            out.append(dict(entry="sam", layout=name, g16=g16, gs=gs, sh=sh))
    for c in out:
        c["id"] = "_".join([c["entry"], c["layout"]] + ["%s%s" % (k, c[k]) for k in ("g16", "gs", "ema_w", "sub", "sh") if k in c])
    return out


def inputs(cfg, seed):
    """-> (dict of fp32 device tensors p, g, m, v, ema, saved over the whole flat buffer, [(offset, numel)] of the tensors): every
    parameter element seeded, every pad a sentinel (v's is positive, like every v), saved a sentinel throughout"""
    import param_tables_ref as tables
    ts, total = tables.tensors(cfg)
    rs = np.random.RandomState(seed)
    elem = np.zeros(total, dtype=bool)
    for off, n, _ in ts:
        elem[off: off + n] = True
    raw = {"p": 0.1 * rs.standard_normal(total), "g": 1e-3 * rs.standard_normal(total), "m": 1e-3 * rs.standard_normal(total),
           "v": (1e-3 * rs.standard_normal(total)) ** 2, "ema": 0.1 * rs.standard_normal(total)}
    x = {}
    for k, a in raw.items():
        a = a.astype(np.float32)
        a[~elem] = SENTINEL
        x[k] = torch.from_numpy(a).to(DEV)
    x["saved"] = torch.full((total,), -SENTINEL, dtype=torch.float32, device=DEV)
    return x, [(off, n) for off, n, _ in ts]


class Digests:
    """one running SHA-256 per named buffer"""

    def __init__(self):
        self.h = {}

    def add(self, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            if t is not None:
                self.h.setdefault(name, hashlib.sha256()).update(t.contiguous().cpu().numpy().tobytes())

    def arrays(self):
        return {name: np.frombuffer(h.digest(), dtype=np.uint8) for name, h in self.h.items()}


def run_case(case):
    """-> {what: array}: a SHA-256 (uint8 [32]) per output buffer over the case's steps, and for sam the records [STEPS, 4] fp32"""
    from mer_amd import runtime
    cfg = layouts()[case["layout"]]
    x, ts = inputs(cfg, 4100 + sum(ord(ch) for ch in case["id"]))
    p, m, v = x["p"], x["m"], x["v"]
    g = x["g"].to(torch.bfloat16) if case.get("g16") else x["g"]
    gs = torch.tensor([GRAD_SCALE], device=DEV) if case.get("gs") else None
    w = case.get("ema_w")
    ema = x["ema"] if (w is not None or case["entry"] == "exchange") else None
    sh = runtime.param_shadow_buffer(cfg, DEV) if (case["entry"] == "shadowed" or case.get("sh")) else None
    first, end = (ts[2][0], ts[-2][0]) if case.get("sub") else (0, -1)
    tg = (ctypes.c_int * len(ts))(*[-1 if i == UNOWNED else i % len(GROUPS) for i in range(len(ts))])
    d, records = Digests(), []
    for step in range(1, STEPS + 1):
        if case["entry"] == "adam":
            runtime.adam_step(p, g, m, v, step, 1e-3, weight_decay=0.01, grad_scale=gs, ema=ema, ema_w=w or 0.0)
            d.add(p=p, m=m, v=v, ema=ema)
        elif case["entry"] == "shadowed":
            runtime.adam_step_shadowed(cfg, p, g, m, v, sh, step, 1e-3, weight_decay=0.01, grad_scale=gs, first=first, end=end,
                                       ema=ema, ema_w=w or 0.0)
            d.add(p=p, m=m, v=v, ema=ema, sh=sh)
        elif case["entry"] == "grouped":
            table = torch.zeros(16, 8, device=DEV)
            runtime.adam_hyper_groups(table, [grp + (step,) for grp in GROUPS])
            runtime.adam_step_grouped(cfg, p, g, m, v, sh, tg, table, grad_scale=gs, first=first, end=end, ema=ema, ema_w=w or 0.0)
            d.add(p=p, m=m, v=v, ema=ema, sh=sh)
        elif case["entry"] == "exchange":
            if step > 2:
                break
            runtime.ema_exchange(cfg, p, ema, tg)
            d.add(p=p, ema=ema)
        elif case["entry"] == "sam":
            scratch, record = runtime.grad_norm_scratch(cfg, DEV), torch.zeros(4, device=DEV)
            runtime.grad_sumsq(cfg, g, scratch)
            runtime.sam_perturb(cfg, p, g, x["saved"], sh, scratch, record, 0.05 * step, gs)
            d.add(p=p, saved=x["saved"], sh=sh)
            records.append(record.cpu().numpy())
            runtime.sam_restore(cfg, p, x["saved"])
            d.add(restored=p)
            p.neg_()                                     # (another point for the next step, exact in every torch)
        else:
            raise ValueError(case["entry"])
    out = d.arrays()
    if records:
        out["record"] = np.stack(records)
    return out


def pack(commit, results):
    """{case id: run_case's dict} -> the fixture's arrays: the digests as ONE [n, 32] array beside their 'id/buffer' keys (an archive
    member per digest would cost ten times the digest), the sam records as one [n, STEPS, 4] array beside their case ids"""
    keys = [(i, k) for i in sorted(results) for k in sorted(results[i]) if k != "record"]
    with_record = [i for i in sorted(results) if "record" in results[i]]
    return {"commit": np.array(commit), "keys": np.array(["%s/%s" % ik for ik in keys]),
            "sha256": np.stack([results[i][k] for i, k in keys]), "record_ids": np.array(with_record),
            "records": np.stack([results[i]["record"] for i in with_record])}


def unpack(fx):
    """the fixture's arrays -> {case id: {what: array}} as run_case gives them"""
    out = {}
    for key, digest in zip(fx["keys"].tolist(), fx["sha256"]):
        i, k = key.split("/")
        out.setdefault(i, {})[k] = digest
    for i, r in zip(fx["record_ids"].tolist(), fx["records"]):
        out[i]["record"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this build was made from (stored in the fixture)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import mer_amd  # noqa: F401
    results = {}
    for case in cases():
        results[case["id"]] = run_case(case)
        print(case["id"], sorted(results[case["id"]]), flush=True)
    np.savez_compressed(args.out, **pack(args.commit, results))
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
