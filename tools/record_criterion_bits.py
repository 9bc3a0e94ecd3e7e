"""Record the bits of the criterion kernels (csrc/rowops.hip: plain, distillation, focal with and without a teacher, R-Drop, and their
finalize / KL-reduce launches) and of the evaluation scoring (csrc/metrics.hip) into tests/golden/criterion_kernel_bits.npz.
tests/test_criterion_kernel_bits_gpu.py regenerates the inputs with the functions of this file and holds every entry to these bits.
The suite's other criterion tests hold the kernels to EACH OTHER's bits (alpha = 0, gamma = 0, eval loss == train loss) and to float64
inside a tolerance; a change that moves all of them together (another summation order, a contracted multiply-add) passes those and
shows here.  The fixture is recorded ONCE, on the commit before such a change; a run that differs from it is a finding about the
kernels, not a reason to record again.

Inputs come from numpy.random.RandomState(seed), whose stream is the same in every numpy version.  One batch per (T, C):
    T in {1, 257} (257 rows: two workgroups, the second with a single live lane), C in {2, 7, 16};
    a batch of 257 (and of 33000) rows holds labels -1 (rows 3, 100), labels >= C (rows 5, 200), rows with a margin of 120 (row 7 on
    its label, row 8 on another class, row 130, and row 9 of the teacher), NaN / +inf / -inf in the teacher rows of the unlabelled rows,
    and a partner map that is a random pairing with one row left at -1, one index >= T and one pair of equal twins (rows copied).
    A batch of one row is one labelled row that is its own twin.
Every entry runs every batch with and without class weights, label_smoothing in {0, 0.1}, normalise in {0, 1} and its own
hyper-parameters: alpha in {0, 0.3}, tau in {1, 2}, gamma in {0, 0.5, 2}.

Stored per (entry, T, C), one row per setting in the order of `settings(entry)`: loss_out [n, 4] and a SHA-256 [n, 32] of the bytes of
dlogits, loss_terms (and the KL terms); the tensors themselves for every setting at T = 1, and at T = 257 for the settings `keeps`
names (class weights, label_smoothing 0.1, normalise 1) - the rest stay digests to keep the file small.  The evaluation cases store
the whole record (eight doubles and the C x C counts) and the row terms in the same way; T = 33000 (more than 128 workgroups of rows:
the rows launch strides) stores the record's eight doubles and a SHA-256 of the terms.

    python tools/record_criterion_bits.py [--out FILE]           (on the GPU; writes the fixture)"""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "criterion_kernel_bits.npz")
DEV = "cuda"
TS, CS = (1, 257), (2, 7, 16)
T_BIG, C_BIG = 33000, 7
ENTRIES = ("plain", "distill", "focal", "focal_teacher", "rdrop")
ALPHAS, TAUS, GAMMAS = (0.0, 0.3), (1.0, 2.0), (0.0, 0.5, 2.0)
UNLABELLED = (3, 100, 5, 200)          # labels -1, -1, C, C + 3


def groups():
    """-> [(entry, T, C)]: one stored block, and one test case, each"""
    return [(e, T, C) for e in ENTRIES + ("eval",) for T in TS for C in CS]


def key(entry, T, C):
    return "%s_T%d_C%d" % (entry, T, C)


def settings(entry):
    """-> list of dicts (cw, ls, norm and the entry's hyper-parameters), in the order the fixture's rows have"""
    hyper = {"plain": [{}],
             "distill": [{"alpha": a, "tau": t} for a in ALPHAS for t in TAUS],
             "focal": [{"gamma": g} for g in GAMMAS],
             "focal_teacher": [{"alpha": a, "tau": t, "gamma": g} for a in ALPHAS for t in TAUS for g in GAMMAS],
             "rdrop": [{"alpha": a} for a in ALPHAS],
             "eval": [{"gamma": None}] + [{"gamma": g} for g in GAMMAS]}[entry]
    norms = (0,) if entry == "eval" else (0, 1)                      # (scoring has no gradient to normalise)
    return [dict(h, cw=cw, ls=ls, norm=norm) for cw, ls, norm in itertools.product((0, 1), (0.0, 0.1), norms) for h in hyper]


def keeps(entry, T, s):
    """whether the tensors of setting s are stored themselves (otherwise their digest alone)"""
    if T == 1:
        return True
    flagship = s["cw"] == 1 and s["ls"] == 0.1 and s["norm"] == (0 if entry == "eval" else 1)
    if entry == "focal_teacher":
        return flagship and s["alpha"] == 0.3 and s["tau"] == 2.0
    return flagship


def inputs(T, C):
    """-> dict of device tensors: logits, teacher [T, C] fp32, labels int64 [T], class_w fp32 [C], partner int32 [T]"""
    rs = np.random.RandomState(7000 + 100 * C + (T % 1000))
    logits = (2.0 * rs.standard_normal((T, C))).astype(np.float32)
    teacher = (2.0 * rs.standard_normal((T, C))).astype(np.float32)
    labels = rs.randint(0, C, size=T).astype(np.int64)
    class_w = (0.5 + rs.rand(C)).astype(np.float32)
    partner = np.zeros(T, dtype=np.int32)                              # T == 1: the row is its own twin
    if T > 1:
        labels[3] = labels[100] = -1
        labels[5], labels[200] = C, C + 3
        logits[7, labels[7]] += 120.0                                  # saturated on its label
        logits[8, (labels[8] + 1) % C] += 120.0                        # ... on another class: a loss of the margin's size
        logits[130] = 0.0
        logits[130, C - 1] = 120.0
        teacher[9, 0] += 120.0
        for r, bad in zip(UNLABELLED, (np.nan, np.inf, -np.inf, np.nan)):
            teacher[r, r % C] = bad
        teacher[3, :] = np.nan
        order = rs.permutation(T)
        partner[:] = -1                                                # (an odd T leaves order[-1] without a twin)
        for i in range(0, T - 1, 2):
            partner[order[i]], partner[order[i + 1]] = order[i + 1], order[i]
        partner[order[0]] = T + 5                                      # an index past the batch: no twin (its twin still reads it)
        # equal twins (s and the KL gradient are exactly 0): the first pair after order[0]'s that touches none of the rows above
        i = next(i for i in range(2, T - 1, 2) if not {order[i], order[i + 1]} & set(UNLABELLED + (7, 8, 9, 130)))
        logits[order[i + 1]] = logits[order[i]]
        labels[order[i + 1]] = labels[order[i]]
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return {"logits": dev(logits), "teacher": dev(teacher), "labels": dev(labels), "class_w": dev(class_w), "partner": dev(partner)}


def sha(*tensors):
    """SHA-256 of the tensors' bytes, one after the other -> uint8 [32]"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def run(entry, x, s):
    """One call of the entry on batch x under setting s -> (loss_out [4], dlogits [T, C], terms [T, 2], kl [T] or None) on the device"""
    from mer_amd.runtime import lib, check, ptr, stream_ptr
    T, C = x["logits"].shape
    cw = x["class_w"] if s["cw"] else None
    terms = torch.full((3 * T,), float("nan"), dtype=torch.float32, device=DEV)
    dl = torch.full((T, C), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.zeros(4, dtype=torch.float32, device=DEV)
    hyper = torch.tensor([s.get("alpha", 0.0), s.get("tau", 1.0), s.get("gamma", 0.0)], dtype=torch.float32).to(DEV)
    common = (ptr(x["labels"]), ptr(cw), s["ls"])
    tail = (s["norm"], ptr(terms), ptr(dl), ptr(out), stream_ptr())
    if entry == "plain":
        check(lib().m2f_cross_entropy(T, C, ptr(x["logits"]), *common, *tail), "m2f_cross_entropy")
    elif entry == "distill":
        check(lib().m2f_cross_entropy_distill(T, C, ptr(x["logits"]), ptr(x["teacher"]), *common, ptr(hyper), *tail),
              "m2f_cross_entropy_distill")
    elif entry in ("focal", "focal_teacher"):
        teacher = x["teacher"] if entry == "focal_teacher" else None
        check(lib().m2f_cross_entropy_focal(T, C, ptr(x["logits"]), ptr(teacher), *common, ptr(hyper), ptr(hyper[2:]), *tail),
              "m2f_cross_entropy_focal")
    elif entry == "rdrop":
        check(lib().m2f_cross_entropy_rdrop(T, C, ptr(x["logits"]), ptr(x["partner"]), *common, ptr(hyper), *tail),
              "m2f_cross_entropy_rdrop")
    else:
        raise ValueError(entry)
    return out, dl, terms[:2 * T].view(T, 2), (terms[2 * T:] if entry == "rdrop" else None)


def run_eval(x, s):
    """m2f_eval_scores (gamma None) or m2f_eval_scores_focal into a zeroed record -> (record float64 [8 + C*C] as stored, terms [T, 2])"""
    from mer_amd.runtime import lib, check, ptr, stream_ptr
    T, C = x["logits"].shape
    cw = x["class_w"] if s["cw"] else None
    record = torch.zeros(lib().m2f_eval_record_bytes(C) // 8, dtype=torch.float64, device=DEV)
    scratch = torch.zeros((lib().m2f_eval_scratch_bytes(T, C) + 7) // 8, dtype=torch.float64, device=DEV)
    if s["gamma"] is None:
        check(lib().m2f_eval_scores(T, C, ptr(x["logits"]), ptr(x["labels"]), ptr(cw), s["ls"], ptr(scratch), ptr(record), stream_ptr()),
              "m2f_eval_scores")
    else:
        g = torch.tensor([s["gamma"]], dtype=torch.float32).to(DEV)
        check(lib().m2f_eval_scores_focal(T, C, ptr(x["logits"]), ptr(x["labels"]), ptr(cw), s["ls"], ptr(g), ptr(scratch), ptr(record),
                                          stream_ptr()), "m2f_eval_scores_focal")
    return record, scratch.view(torch.float32)[:2 * T].view(T, 2)


def big_settings():
    return [{"gamma": None, "cw": 1, "ls": 0.1}, {"gamma": 2.0, "cw": 1, "ls": 0.1}]


def record_group(entry, T, C):
    """-> dict of the arrays stored for one (entry, T, C), keyed '<key>/<what>'"""
    x = inputs(T, C)
    k = key(entry, T, C)
    heads, digests, kept = [], [], {"dlogits": [], "terms": [], "kl": []}
    for s in settings(entry):
        if entry == "eval":
            head, terms = run_eval(x, s)
            parts = {"terms": terms}
        else:
            head, dl, terms, kl = run(entry, x, s)
            parts = {"dlogits": dl, "terms": terms}
            if kl is not None:
                parts["kl"] = kl
        heads.append(head.cpu().numpy())
        digests.append(sha(*parts.values()))
        if keeps(entry, T, s):
            for name, t in parts.items():
                kept[name].append(t.cpu().numpy())
    out = {k + ("/record" if entry == "eval" else "/loss_out"): np.stack(heads), k + "/sha256": np.stack(digests)}
    out.update({k + "/" + name: np.stack(v) for name, v in kept.items() if v})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import mer_amd  # noqa: F401
    fx = {}
    for entry, T, C in groups():
        got = record_group(entry, T, C)
        fx.update(got)
        print(key(entry, T, C), {n.split("/")[1]: a.shape for n, a in got.items()}, flush=True)
    x = inputs(T_BIG, C_BIG)
    heads, digests = zip(*((r[:8].cpu().numpy(), sha(t)) for r, t in (run_eval(x, s) for s in big_settings())))
    fx[key("eval", T_BIG, C_BIG) + "/record"], fx[key("eval", T_BIG, C_BIG) + "/sha256"] = np.stack(heads), np.stack(digests)
    print(key("eval", T_BIG, C_BIG), np.stack(heads)[:, 4], flush=True)
    np.savez_compressed(args.out, **fx)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
