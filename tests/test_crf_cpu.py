"""Host-side checks of the linear-chain CRF: the float64 reference (tests/golden/crf_ref.py) against brute-force enumeration of every
path, its zero-parameter case against the plain criterion, `LinearChainCRF.from_label_counts`, the parameter block's layout, the host
refusals, and the share of rounding-decided positions in the Viterbi inputs the GPU tests use.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import crf_cases as cases
import crf_ref as ref
import mer_amd  # noqa: F401
from mer_amd.crf import LinearChainCRF, label_count_params, param_count


@pytest.mark.parametrize("C,L", [(7, 1), (7, 2), (7, 5), (3, 8), (2, 10)])
def test_recursion_equals_enumeration(C, L):
    g = torch.Generator().manual_seed(10 * C + L)
    e = torch.randn(L, C, generator=g, dtype=torch.float64) * 2.0
    params = cases.params_block(C, 20 * C + L).double()
    brute = ref.enumerate_paths(e, params)
    marg, pairs, logZ = ref.marginals(e, params)
    path, score, gaps = ref.viterbi(e, params)
    figs = (abs(float(ref.log_z(e, params) - brute["logZ"])), abs(float(logZ - brute["logZ"])),
            float((marg - brute["marginals"]).abs().max()), float((pairs - brute["pairs"]).abs().max()) if L > 1 else 0.0)
    print(f"C={C} L={L}: logZ err {figs[0]:.3g} / {figs[1]:.3g}, marginals {figs[2]:.3g}, pair marginals {figs[3]:.3g}; "
          f"best {brute['best']} score {float(brute['best_score']):.12g} viterbi {path} {float(score):.12g}")
    assert max(figs) <= 1e-12
    assert path == brute["best"]
    assert abs(float(score - brute["best_score"])) <= 1e-12 * max(1.0, abs(float(score)))
    assert (gaps >= 0).all()
    # the gradient of logZ under autograd is the marginal
    ez = e.clone().requires_grad_(True)
    (dz,) = torch.autograd.grad(ref.log_z(ez, params), ez)
    assert float((dz - brute["marginals"]).abs().max()) <= 1e-12


def test_zero_parameters_are_the_sum_of_row_criteria():
    """At zero parameters logZ - score(y) is the sum of the rows' cross entropies (to float64 rounding: the recursion adds
    logsumexp(alpha) row by row where the criterion adds the rows' own)."""
    c = cases.nll_case(7, 4, 64, False, seed=5)
    zero = torch.zeros_like(c["params"])
    num, den, _ = ref.nll(c["logits"].double(), c["labels"], zero, c["spans"])
    ce = TF.cross_entropy(c["logits"].double(), c["labels"], ignore_index=-1, reduction="sum")
    print(f"zero parameters: num {float(num):.15g} sum of CE {float(ce):.15g} den {den}")
    assert den == int((c["labels"] >= 0).sum())
    assert abs(float(num - ce)) <= 1e-12 * abs(float(ce))
    loss, dz, dp = ref.nll_grads(c["logits"], c["labels"], zero, c["spans"])
    zz = c["logits"].double().requires_grad_(True)
    TF.cross_entropy(zz, c["labels"], ignore_index=-1).backward()
    assert float((dz - zz.grad).abs().max()) <= 1e-14


def test_unlabelled_rows_link_their_neighbours():
    """A -1 in the middle: the loss is that of the chain with the row removed; a dialogue without a label adds nothing."""
    c = cases.nll_case(3, 5, 17, True, seed=8)
    num, den, nums = ref.nll(c["logits"].double(), c["labels"], c["params"], c["spans"])
    keep = c["labels"] >= 0
    # the same chains as one span each over the labelled rows only
    z2, y2 = c["logits"][keep], c["labels"][keep]
    idx = torch.cumsum(keep.long(), 0) - 1
    spans2 = []
    for r0, r1 in c["spans"]:
        rows = torch.arange(r0, r1)[keep[r0:r1]]
        if rows.numel():
            spans2.append((int(idx[rows[0]]), int(idx[rows[-1]]) + 1))
    num2, den2, _ = ref.nll(z2.double(), y2, c["params"], spans2)
    assert den == den2 and float(num) == float(num2) and len(nums) == len(spans2) < len(c["spans"])


@pytest.mark.parametrize("smoothing", [1.0, 0.25])
def test_from_label_counts(smoothing):
    C = 7
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(1, 25, (40,), generator=g)
    labels = torch.randint(0, C - 1, (int(lengths.sum()),), generator=g)          # class 6 never occurs: only smoothing keeps it finite
    labels[torch.rand(labels.numel(), generator=g) < 0.2] = -1
    crf = LinearChainCRF.from_label_counts(labels.numpy(), lengths.numpy(), smoothing, num_classes=C)
    tr, st, en = crf.transitions.detach(), crf.start.detach(), crf.end.detach()
    print("row sums of exp(transitions):", tr.exp().sum(1).tolist(), "start", float(st.exp().sum()), "end", float(en.exp().sum()))
    assert torch.isfinite(crf.params).all()
    assert torch.allclose(tr.exp().sum(1), torch.ones(C), atol=1e-6)
    assert abs(float(st.exp().sum()) - 1) <= 1e-6 and abs(float(en.exp().sum()) - 1) <= 1e-6
    # the counts themselves, on a set small enough to count by hand: dialogues (0, 1, -1, 1) and (2,)
    blk = label_count_params([0, 1, -1, 1, 2], [4, 1], 3, smoothing=1.0)
    t = np.exp(blk[:9].reshape(3, 3).astype(np.float64))
    assert np.allclose(t[0], [1 / 4, 2 / 4, 1 / 4], atol=1e-6) and np.allclose(t[1], [1 / 4, 2 / 4, 1 / 4], atol=1e-6)       # 0->1, 1->1 (linked)
    assert np.allclose(np.exp(blk[9:12].astype(np.float64)), [2 / 5, 1 / 5, 2 / 5], atol=1e-6)                              # starts: 0, 2
    assert np.allclose(np.exp(blk[12:].astype(np.float64)), [1 / 5, 2 / 5, 2 / 5], atol=1e-6)                               # ends: 1, 2
    with pytest.raises(ValueError, match="lengths"):
        label_count_params([0, 1], [3], 3)
    with pytest.raises(ValueError, match="labels"):
        label_count_params([0, 3], [2], 3)


def test_parameter_block_layout():
    for C in (2, 7, 16):
        crf = LinearChainCRF(C)
        assert crf.params.dtype == torch.float32 and crf.params.numel() == param_count(C) == C * C + 2 * C
        assert crf.params.data_ptr() % 16 == 0 and (crf.params == 0).all() and crf.trainable
        assert list(dict(crf.named_parameters())) == ["params"]
        with torch.no_grad():
            crf.params.copy_(torch.arange(param_count(C), dtype=torch.float32))
        assert crf.transitions[1, 0] == C and crf.start[0] == C * C and crf.end[0] == C * C + C and crf.end[-1] == param_count(C) - 1
        assert crf.transitions.data_ptr() == crf.params.data_ptr()                 # views, not copies
        crf.params.requires_grad_(False)
        assert not crf.trainable
    for bad in (1, 17, 7.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            LinearChainCRF(bad)
    crf = LinearChainCRF(7)
    with pytest.raises(ValueError, match="neither"):
        crf._rows(torch.zeros(2, 5, 6), torch.zeros(2, 5, dtype=torch.long), "forward")
    assert crf._rows(torch.zeros(2, 7, 5), torch.zeros(2, 5), "forward").shape == (2, 5, 7)
    assert crf._rows(torch.zeros(2, 5, 7), torch.zeros(2, 5), "forward").shape == (2, 5, 7)


def test_viterbi_inputs_are_decided_by_more_than_rounding():
    """The Viterbi inputs of tests/test_crf_kernels_gpu.py: at most 1 % of the positions have a float64 max-marginal gap under 1e-3
    (those are left out of the label comparison there)."""
    for L in cases.VITERBI_L:
        logits, mask, params = cases.viterbi_case(L)
        small = total = 0
        for b in range(logits.shape[0]):
            rows = torch.nonzero(~mask[b]).flatten()
            if rows.numel() == 0:
                continue
            _, _, gaps = ref.viterbi(logits[b, rows], params)
            small += int((gaps <= cases.GAP).sum())
            total += gaps.numel()
        print(f"L={L}: {small} of {total} positions under the gap ({small / max(total, 1):.3%})")
        assert small <= cases.MAX_EXCLUDED * total


def test_step_refusals_name_their_pair():
    """`crf=` beside anything the CRF criterion has no form for is a ValueError on the host, before any launch."""
    from mer_amd.criterion import PLAIN, resolve

    def check_step_args(who, crf, num_classes, class_weights=None, label_smoothing=0.0, **kw):
        return resolve(who, num_classes=num_classes, cls_hidden=64, mask_shape=(1, 1), device="cpu", label_smoothing=label_smoothing,
                       class_weights=class_weights, crf=crf, **kw)
    crf = LinearChainCRF(7)
    assert check_step_args("train_step", None, 7, class_weights=torch.ones(7), label_smoothing=0.1) is PLAIN          # no crf: nothing to refuse
    assert check_step_args("train_step", crf, 7).crf is crf
    for kw, name in (({"class_weights": torch.ones(7)}, "class_weights"), ({"teacher_logits": torch.zeros(1)}, "teacher_logits / distill"),
                     ({"distill": (0.5, 2.0)}, "teacher_logits / distill"), ({"focal_gamma": 0.0}, "focal_gamma"),
                     ({"label_smoothing": 0.1}, "label_smoothing != 0.0")):
        with pytest.raises(ValueError, match="train_step: crf= does not combine with " + name):
            check_step_args("train_step", crf, 7, **kw)
    with pytest.raises(ValueError, match="7 classes, the model's classifier has 4"):
        check_step_args("train_step", crf, 4)
    with pytest.raises(ValueError, match="must be a LinearChainCRF"):
        check_step_args("train_step", torch.zeros(63), 7)
    with pytest.raises(ValueError, match="trainable crf= does not combine with gradient accumulation"):
        check_step_args("train_step", crf, 7, accumulating=True)
    with pytest.raises(ValueError, match="trainable crf= does not combine with DataParallelStep"):
        check_step_args("DataParallelStep", crf, 7, data_parallel=True)
    # an evaluation step writes no gradient: a trainable block is an input there, whatever the training mode
    assert check_step_args("M2FNet.eval_step", crf, 7, evaluating=True, accumulating=True).crf is crf
    assert check_step_args("M2FNet.eval_step", crf, 7, evaluating=True, accumulating=True, data_parallel=True, focal_gamma=None).crf is crf
    with pytest.raises(ValueError, match="eval_step: crf= does not combine with focal_gamma"):
        check_step_args("M2FNet.eval_step", crf, 7, evaluating=True, accumulating=True, focal_gamma=2.0)
    crf.params.requires_grad_(False)                      # frozen: a pure input, fine under both
    assert check_step_args("train_step", crf, 7, accumulating=True, data_parallel=True).crf is crf
    with pytest.raises(ValueError, match="move the module"):
        crf.block("cuda:0")


def test_runtime_crf_keys_in_the_config():
    """src/config.yaml carries the `runtime.crf` block with its four keys and their defaults, `solver.loss_fn` names CRF, and
    train.crf_settings reads and checks the block on the host."""
    import os
    import sys
    import yaml
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    with open(os.path.join(root, "src", "config.yaml")) as f:
        text = f.read()
    cfg = yaml.safe_load(text)
    assert cfg["runtime"]["crf"] == {"init": "zeros", "smoothing": 1.0, "trainable": True, "lr": 1.0e-2}
    assert "crf" not in cfg["solver"] and "CRF" in [ln for ln in text.splitlines() if ln.strip().startswith("loss_fn:")][0]
    sys.path.insert(0, os.path.join(root, "src"))
    import train as tr
    assert tr.crf_settings(cfg) == {"init": "zeros", "smoothing": 1.0, "trainable": True, "lr": 1.0e-2}
    assert tr.crf_settings({"runtime": {}})["init"] == "zeros"
    assert tr.crf_settings({"runtime": {"crf": {"init": "bigram", "trainable": False}}}) == {"init": "bigram", "smoothing": 1.0,
                                                                                            "trainable": False, "lr": 1.0e-2}
    for block, name in (({"init": "ones"}, "init"), ({"smoothing": -1.0}, "smoothing"), ({"lr": 0}, "lr"), ({"trainable": 1}, "trainable"),
                        ({"gamma": 2.0}, "unknown key")):
        with pytest.raises(ValueError, match="runtime.crf.*" + name):
            tr.crf_settings({"runtime": {"crf": block}})
    assert tr.CRF_KEY == "crf_state_dict"
