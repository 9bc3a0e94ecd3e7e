"""The criterion kernels (csrc/rowops.hip: plain, distillation, focal with and without a teacher, R-Drop, their finalize and KL-reduce
launches) and the evaluation scoring (csrc/metrics.hip) against the bits recorded in tests/golden/criterion_kernel_bits.npz by
tools/record_criterion_bits.py, on the commit before the six copies of the criterion row became one definition (csrc/criterion_row.h).
The other criterion tests hold these kernels to each other's bits and to float64 inside a tolerance, which a change that moves them
all together would pass.  Here every batch and every setting - the lists and the input generator are the recording tool's - must give
the recorded loss_out, dlogits, loss_terms and KL terms bit for bit (the tensors where the fixture keeps them, their SHA-256
everywhere).  A difference is a change in what the kernels compute: the fixture is not recorded again."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_criterion_bits as rec  # noqa: E402

GROUPS = rec.groups()
BIG = rec.key("eval", rec.T_BIG, rec.C_BIG)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "criterion_kernel_bits.npz"), allow_pickle=False)


def same_bits(got, want):
    """torch.equal on the integer views: a NaN equals itself, -0 does not equal 0"""
    got, want = torch.as_tensor(got).cpu().contiguous(), torch.from_numpy(np.ascontiguousarray(want))
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    view = {torch.float32: torch.int32, torch.float64: torch.int64}.get(got.dtype, got.dtype)
    return torch.equal(got.view(view), want.view(view))


def test_the_cases_are_the_ones_recorded(recorded):
    assert len(GROUPS) == 36 and {g[0] for g in GROUPS} == set(rec.ENTRIES) | {"eval"}
    assert [len(rec.settings(e)) for e in rec.ENTRIES + ("eval",)] == [8, 32, 24, 96, 16, 16]
    want = {BIG + "/record", BIG + "/sha256"}
    for entry, T, C in GROUPS:
        k = rec.key(entry, T, C)
        want |= {k + ("/record" if entry == "eval" else "/loss_out"), k + "/sha256", k + "/terms"}
        want |= {k + "/dlogits"} if entry != "eval" else set()
        want |= {k + "/kl"} if entry == "rdrop" else set()
        kept = sum(rec.keeps(entry, T, s) for s in rec.settings(entry))
        assert kept >= 1 and recorded[k + "/terms"].shape == (kept, T, 2)
        assert recorded[k + "/sha256"].shape == (len(rec.settings(entry)), 32)
    assert set(recorded.files) == want


@pytest.mark.parametrize("group", GROUPS, ids=[rec.key(*g) for g in GROUPS])
def test_the_bits_are_the_recorded_ones(recorded, group):
    entry, T, C = group
    k = rec.key(entry, T, C)
    x = rec.inputs(T, C)
    head_name = "record" if entry == "eval" else "loss_out"
    wrong, kept = [], 0
    for i, s in enumerate(rec.settings(entry)):
        if entry == "eval":
            head, terms = rec.run_eval(x, s)
            parts = {"terms": terms}
        else:
            head, dl, terms, kl = rec.run(entry, x, s)
            parts = {"dlogits": dl, "terms": terms}
            if kl is not None:
                parts["kl"] = kl
        if not same_bits(head, recorded[k + "/" + head_name][i]):
            wrong.append((i, s, head_name, head.tolist(), recorded[k + "/" + head_name][i].tolist()))
        if rec.keeps(entry, T, s):
            for name, t in parts.items():
                if not same_bits(t, recorded[k + "/" + name][kept]):
                    diff = (t.cpu() != torch.from_numpy(recorded[k + "/" + name][kept])).sum().item()
                    wrong.append((i, s, name, "%d of %d values differ" % (diff, t.numel())))
            kept += 1
        if not same_bits(torch.from_numpy(rec.sha(*parts.values()).copy()), recorded[k + "/sha256"][i]):
            wrong.append((i, s, "sha256 of " + " + ".join(parts)))
    assert not wrong, "%d differences from the recorded bits, the first: %r" % (len(wrong), wrong[0])


@pytest.mark.parametrize("i", [0, 1], ids=["plain", "focal"])
def test_the_strided_rows_launch_gives_the_recorded_bits(recorded, i):
    """T = 33000: 129 blocks of rows asked for, 128 launched - the rows kernel strides"""
    s = rec.big_settings()[i]
    record, terms = rec.run_eval(rec.inputs(rec.T_BIG, rec.C_BIG), s)
    assert same_bits(record[:8], recorded[BIG + "/record"][i]), (record[:8].tolist(), recorded[BIG + "/record"][i].tolist())
    assert same_bits(torch.from_numpy(rec.sha(terms).copy()), recorded[BIG + "/sha256"][i])
