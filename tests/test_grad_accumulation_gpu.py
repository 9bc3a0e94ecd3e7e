"""Gradient accumulation over micro-batches (M2FNet.set_grad_accumulation, m2f_plan_accumulate_grads): the accumulate form of every
launch that writes a parameter gradient adds old + new in one rounded fp32 add, so k accumulating backwards leave exactly the fp32 sum
of the k overwrite-form gradients - checked with torch.equal, per parameter, on three plan kinds that share one gradient buffer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, M2FCrossEntropyLoss  # noqa: E402

CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2)          # dropout 0


def _model(precision="fp32"):
    m = M2FNet(CFG, precision=precision)
    m.load_state_dict(synth.make_state_dict(CFG))
    return m.to("cuda").train()


def _batch(B, L, seed, lengths=None):
    if lengths is None:
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
    return [t.cuda() for t in synth.make_inputs(CFG, B, L, lengths, "randn", seed=seed)]


def _micro_batches():
    # two L-buckets of padded plans and one long dialogue (L = 80 > 64: a packed plan)
    return {"A": _batch(8, 16, 1), "B": _batch(8, 32, 2), "C": _batch(2, 80, 3, lengths=[80, 23])}


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _tail(m):
    return m.loss_terms()[1:].detach().clone()


def _check_sum(m, refs, names, what):
    tot = None
    for n in names:
        tot = refs[n] if tot is None else {k: tot[k] + refs[n][k] for k in tot}
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, tot[k]), (what, k, (p.grad - tot[k]).abs().max().item())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("variant", ["default", "table131", "wgrad_grouped"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_accumulation_is_the_fp32_sum(precision, variant, use_graph, monkeypatch):
    if variant == "table131":
        monkeypatch.setenv("M2F_TABLE_TILE", "131")
    elif variant == "wgrad_grouped":
        monkeypatch.setenv("M2F_WGRAD_TABLE", "0")
    m = _model(precision)
    mbs = _micro_batches()
    refs, tails = {}, {}
    for _ in range(2):                                     # overwrite form (the second round replays its graphs)
        for n, mb in mbs.items():
            m.zero_grad(set_to_none=True)
            m.train_step(*mb, use_graph=use_graph)
            refs[n], tails[n] = _grads(m), _tail(m)
    m.set_grad_accumulation(True)
    for group in (["A", "B", "C"], ["A", "B"], ["C", "A", "B"]):
        m.zero_grad(set_to_none=True)
        for n in group:
            loss = m.train_step(*mbs[n], use_graph=use_graph)
            assert loss.item() == m.loss_terms()[0].item()
        torch.cuda.synchronize()
        _check_sum(m, refs, group, group)
        want = tails[group[0]]
        for n in group[1:]:
            want = want + tails[n]
        assert torch.equal(_tail(m), want), (group, _tail(m), want)
    # both forms of every plan stay in the one graph cache: back to the overwrite form, same bits as before
    m.set_grad_accumulation(False)
    for n, mb in mbs.items():
        m.train_step(*mb, use_graph=use_graph)
        torch.cuda.synchronize()
        _check_sum(m, refs, [n], "off again " + n)


# 256-wide model: every weight gradient of the encoders, the fusion stack and the classifier is at least 256 x 256, so the table
# launches run their WHOLE-tile accumulate epilogues (eight-phase: 256 x 256 tiles with the vectorised old-dW loads; ring form:
# 256 x 128 tiles through the LDS image with the accumulate term) - the narrow CFG above reaches only their edge-tile code
CFG_WIDE = synth._cfg(256, 256, 256, 4, 4, 4, 1, 1, 1)


@pytest.mark.parametrize("variant", ["default", "table131"])
def test_train_step_accumulation_whole_tiles_bf16(variant, monkeypatch):
    if variant == "table131":
        monkeypatch.setenv("M2F_TABLE_TILE", "131")
    m = M2FNet(CFG_WIDE, precision="bf16")
    m.load_state_dict(synth.make_state_dict(CFG_WIDE))
    m = m.to("cuda").train()
    mbs = {}
    for n, (B, L, seed) in {"A": (8, 16, 21), "B": (16, 32, 22), "C": (8, 32, 23)}.items():
        g = torch.Generator().manual_seed(seed)
        lengths = [L] + [int(x) for x in torch.randint(1, L + 1, (B - 1,), generator=g)]
        mbs[n] = [t.cuda() for t in synth.make_inputs(CFG_WIDE, B, L, lengths, "randn", seed=seed)]
    refs = {}
    for _ in range(2):
        for n, mb in mbs.items():
            m.zero_grad(set_to_none=True)
            m.train_step(*mb)
            refs[n] = _grads(m)
    assert any(min(p.shape) >= 256 for p in m.parameters() if p.dim() == 2)
    m.set_grad_accumulation(True)
    for group in (["A", "B", "C"], ["C", "A"]):
        m.zero_grad(set_to_none=True)
        for n in group:
            m.train_step(*mbs[n])
        torch.cuda.synchronize()
        _check_sum(m, refs, group, group)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_switch_off_restores_the_overwrite_form_for_the_optimizer_step(precision):
    """After a group in the accumulate form, set_grad_accumulation(False) puts every plan back in the overwrite form: a following
    train_step(optimizer=...) (fp32: the optimizer's own kernel behind the step; bf16: Adam in the weight-gradient launch) leaves
    the same parameters, bit for bit, as on a model that never accumulated."""
    mbs = _micro_batches()
    m_acc, m_ref = _model(precision), _model(precision)
    m_acc.set_grad_accumulation(True)
    m_acc.zero_grad(set_to_none=True)
    for n in ("A", "B", "A"):
        m_acc.train_step(*mbs[n])
    m_acc.set_grad_accumulation(False)
    o_acc, o_ref = FusedAdam(m_acc, lr=1e-3, weight_decay=0.01), FusedAdam(m_ref, lr=1e-3, weight_decay=0.01)
    for _ in range(2):
        for n in ("A", "B"):
            o_acc.zero_grad()
            o_ref.zero_grad()
            la = m_acc.train_step(*mbs[n], optimizer=o_acc).item()
            lr_ = m_ref.train_step(*mbs[n], optimizer=o_ref).item()
            assert la == lr_, (n, la, lr_)
    torch.cuda.synchronize()
    for (k, p), (_, q) in zip(m_acc.named_parameters(), m_ref.named_parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(m_acc.loss_terms(), m_ref.loss_terms())


def test_accumulate_form_stays_on_across_a_plan_rebuild():
    """A rebuild of a plan's launch lists (m2f_plan_backward_outputs, there and back) while the plan is in the accumulate form: the form
    stays on and its lists follow the rebuild - two micro-batches accumulated afterwards, captured step included, leave bit for bit the
    gradients and the criterion tail of a plan that never rebuilt."""
    cfg, B, L, lengths, kind = synth.CASES["tiny_ragged"]
    mbs = [[t.cuda() for t in synth.make_inputs(cfg, B, L, lengths, kind, seed=s)] for s in (11, 12)]

    def run(rebuild):
        m = M2FNet(cfg, precision="bf16")
        m.load_state_dict(synth.make_state_dict(cfg))
        m = m.to("cuda").train()
        m.set_grad_accumulation(True)
        m.zero_grad(set_to_none=True)
        for mb in mbs + mbs:                                 # (the first one overwrites; the accumulate form is captured after it)
            m.train_step(*mb, use_graph=True)
        torch.cuda.synchronize()
        plan = next(iter(m.engine().plans.values()))
        assert plan._acc
        if rebuild:
            plan.backward_outputs(3, True)
            plan.backward_outputs(0, True)
            assert plan._acc
        out = []
        for _ in range(2):                                   # (after a rebuild: one eager round, one captured)
            m.zero_grad(set_to_none=False)                   # the engine's views, zeroed: both micro-batches accumulate
            for mb in mbs:
                m.train_step(*mb, use_graph=True)
            torch.cuda.synchronize()
            out.append((_grads(m), _tail(m)))
        return out
    for (ga, ta), (gb, tb) in zip(run(True), run(False)):
        assert torch.equal(ta, tb), (ta, tb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), (k, (ga[k] - gb[k]).abs().max().item())
        assert any(bool((g != 0).any()) for g in ga.values())


def _autograd_grads(m, mb, crit):
    t, a, kp, em = mb
    loss = crit(m(t, a, kp).permute(0, 2, 1), em)
    loss.backward()
    torch.cuda.synchronize()


def test_loss_backward_follows_torch_grad_rule():
    m = _model("fp32")
    crit = M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    A, B2 = _batch(8, 16, 4), _batch(8, 16, 5)              # one bucket
    refs = {}
    for n, mb in (("A", A), ("B", B2)):
        m.zero_grad(set_to_none=True)
        _autograd_grads(m, mb, crit)
        refs[n] = _grads(m)
    # switch off: the second backward overwrites
    m.zero_grad(set_to_none=True)
    _autograd_grads(m, A, crit)
    _autograd_grads(m, B2, crit)
    _check_sum(m, refs, ["B"], "off")
    m.set_grad_accumulation(True)
    for set_to_none in (True, False):
        m.zero_grad(set_to_none=set_to_none)
        _autograd_grads(m, A, crit)
        _autograd_grads(m, B2, crit)
        _check_sum(m, refs, ["A", "B"], f"set_to_none={set_to_none}")
    # one parameter's .grad set to None: it takes the fresh gradient, the others the sum
    m.zero_grad(set_to_none=True)
    _autograd_grads(m, A, crit)
    name0, p0 = next(iter(m.named_parameters()))
    p0.grad = None
    _autograd_grads(m, B2, crit)
    for k, p in m.named_parameters():
        want = refs["B"][k] if k == name0 else refs["A"][k] + refs["B"][k]
        assert torch.equal(p.grad, want), k
    # two live forwards of one bucket (two plan instances), then both backwards
    m.zero_grad(set_to_none=True)
    (t1, a1, k1, e1), (t2, a2, k2, e2) = A, B2
    out_a = m(t1, a1, k1)
    out_b = m(t2, a2, k2)
    crit(out_a.permute(0, 2, 1), e1).backward()
    crit(out_b.permute(0, 2, 1), e2).backward()
    torch.cuda.synchronize()
    _check_sum(m, refs, ["A", "B"], "two instances")


def test_global_denominator_equals_one_big_batch():
    """Four micro-batches of 8 ragged dialogues with normalise=False, summed and divided by the group's den, against one train_step
    on the 32-dialogue concatenation.  Only the summation order differs (per micro-batch partial sums of the weight-gradient
    reductions and the criterion's den / num).  Measured on MI355X: gradient error 9.8e-7 of the largest gradient element of its
    tensor; the bound below leaves a factor five."""
    torch.manual_seed(0)
    big = _batch(32, 16, 9)
    mbs = [[x[i * 8:(i + 1) * 8] for x in big] for i in range(4)]
    m_big, m_acc = _model("fp32"), _model("fp32")
    m_acc.set_grad_accumulation(True)
    loss_big = m_big.train_step(*big, use_graph=False)
    m_acc.zero_grad(set_to_none=True)
    for mb in mbs:
        m_acc.train_step(*mb, normalise=False, use_graph=False)
    den, num = m_acc.loss_terms()[1], m_acc.loss_terms()[2]
    assert abs((num / den).item() - loss_big.item()) < 1e-5
    worst = 0.0
    for (k, p), (_, q) in zip(m_acc.named_parameters(), m_big.named_parameters()):
        err = ((p.grad / den) - q.grad).abs().max().item() / max(q.grad.abs().max().item(), 1e-12)
        worst = max(worst, err)
    print(f"global-denominator gradient error (relative to the largest element): {worst:.3e}")
    assert worst < 5e-6, worst
    # three optimizer steps of each: same loss trajectory within the 1e-4 of the Adam trajectory tests
    o_big = FusedAdam(m_big, lr=1e-3, weight_decay=0.01)
    o_acc = FusedAdam(m_acc, lr=1e-3, weight_decay=0.01)
    for _ in range(3):
        o_big.zero_grad()
        lb = m_big.train_step(*big, use_graph=False).item()
        o_big.step()
        o_acc.zero_grad()
        for mb in mbs:
            m_acc.train_step(*mb, normalise=False, use_graph=False)
        terms = m_acc.loss_terms()
        la = (terms[2] / terms[1]).item()
        o_acc.grad_scale = terms[1:2]
        o_acc.step()
        assert abs(la - lb) < 1e-4, (la, lb)


def test_refusals():
    m = _model("bf16")
    mb = _batch(8, 16, 1)
    m.train_step(*mb, use_graph=False)
    m.set_grad_accumulation(True)
    with pytest.raises(RuntimeError, match="bf16 gradients"):
        m.set_grad_bf16(True)
    with pytest.raises(RuntimeError, match="optimizer"):
        m.train_step(*mb, optimizer=FusedAdam(m, lr=1e-3))
    pl = next(p for p in m.engine().plans.values() if p.train)
    pl.accumulate_grads(True)
    with pytest.raises(runtime.HipError, match="split step has no accumulate form"):
        pl.step_part(0, use_graph=False)
    m.set_grad_accumulation(False)
    pl.accumulate_grads(False)
    assert m.set_grad_bf16(True)
    with pytest.raises(RuntimeError, match="bf16 gradients are on"):
        m.set_grad_accumulation(True)
    with pytest.raises(runtime.HipError, match="bf16 gradients are armed"):
        pl.accumulate_grads(True)


def _dataset(n_dia, d_t, d_a, seed):
    import numpy as np
    import pandas as pd
    import dataset as ds
    g = np.random.default_rng(seed)
    rows = [(f"utt {d}-{u}", list(ds.EMOTIONS)[int(g.integers(0, 7))], d, u) for d in range(n_dia) for u in range(int(g.integers(1, 10)))]
    table = pd.DataFrame(rows, columns=["Utterance", "Emotion", "Dialogue_ID", "Utterance_ID"])
    text = torch.from_numpy(g.standard_normal((len(rows), d_t)).astype(np.float32))
    audio = torch.from_numpy(g.standard_normal((len(rows), d_a)).astype(np.float32))
    return ds.Dataset("train", text_embeddings=text, audio_embeddings=audio, table=table)


def test_train_loop_grad_accumulation_equals_hand_loop(monkeypatch):
    """src/train.py with runtime.grad_accumulation: 2 (one epoch, synthetic MELD-shaped data, last group shorter) leaves the same
    parameters, bit for bit, as a hand-written loop doing the same grouping."""
    import os
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "src"))
    monkeypatch.chdir(root)
    import dataset as ds
    import train as tr
    from utils import AttrDict
    cfg = AttrDict(runtime=AttrDict(grad_accumulation=2))
    k = tr.grad_accumulation_steps(cfg, 1)
    model_cfg = AttrDict(synth._cfg(40, 48, 64, 4, 4, 4, 1, 1, 1))
    d_train = _dataset(36, 48, 40, 1)
    dl = torch.utils.data.DataLoader(d_train, collate_fn=ds.collate_fn, batch_size=8, shuffle=False)
    assert len(dl) % k == 1                                # the last group holds one batch
    device = torch.device("cuda:0")
    crit = tr.M2FCrossEntropyLoss(ignore_index=-1, label_smoothing=0.1)
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(tr.M2FNet(model_cfg).to(device))
    m_loop, m_hand = models
    m_loop.grad_accumulation_k = k
    o_loop = tr.FusedAdam(m_loop, lr=2e-3, weight_decay=0.01)
    mean = tr.train(m_loop, dl, crit, o_loop, 0, False, device)
    o_hand = tr.FusedAdam(m_hand, lr=2e-3, weight_decay=0.01)
    m_hand.set_grad_accumulation(True)
    losses = []
    batches = list(dl)
    for g0 in range(0, len(batches), k):
        o_hand.zero_grad()
        for batch in batches[g0:g0 + k]:
            text, audio, emotion, pad = tr.move_batch(batch, device)
            m_hand.train_step(text, audio, pad, emotion, label_smoothing=0.1, normalise=False)
        terms = m_hand.loss_terms()
        o_hand.grad_scale = terms[1:2]
        o_hand.step()
        losses.append((terms[2] / terms[1]).item())
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(m_loop.named_parameters(), m_hand.named_parameters()):
        assert torch.equal(p, q), n
    assert abs(mean - sum(losses) / len(losses)) < 1e-6
