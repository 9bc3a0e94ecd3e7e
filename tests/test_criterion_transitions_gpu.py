"""Plan.set_criterion across every change of criterion: one model steps through a walk that contains every ordered pair of the nine
criteria a step can ask for (plain, distill, focal, distill+focal, crf, rdrop, supcon, aux, aux+focal), and after every step the
criterion tail (loss, den, num and the fourth float) holds the bits that criterion gave a model that had run nothing else - whatever
the plan held before.  No optimizer: the weights never change; the CRF's and the head's blocks are frozen, every hyper-parameter is
fixed.  The walk runs eagerly and with use_graph=True, where every change of a switch drops the captured step and captures again, and
each visit steps twice: the second call finds its criterion held and replays.  R-Drop runs in the plan of 2B dialogues; plain and
focal steps on a batch of 8 enter that plan with R-Drop's switch held, and R-Drop enters it with theirs.

The tail is zeroed in front of every step: only R-Drop, supcon and aux write its fourth float, so after a step of any other criterion
it reads 0 - unless a term that should be off still ran."""
import itertools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd.aux_head import AuxiliaryHead  # noqa: E402
from mer_amd.crf import LinearChainCRF  # noqa: E402
from mer_amd.metrics import DeviceScores  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_criterion_switches_gpu.py's rig)
C, A, B, L, LENGTHS = 7, 3, 4, 6, [6, 6, 5, 6]
NINE = ("plain", "distill", "focal", "distill+focal", "crf", "rdrop", "supcon", "aux", "aux+focal")
EIGHT = ("plain8", "focal8")                                     # the 4 dialogues twice: R-Drop's plan, without R-Drop


def _model():
    m = M2FNet(CFG, precision="fp32")
    m.load_state_dict(synth.make_state_dict(CFG))
    return m.to(DEV).train()


def euler_walk(n):
    """A closed walk over n states that takes every ordered pair of distinct states exactly once (Hierholzer on the complete digraph)"""
    out = {v: [u for u in range(n) if u != v] for v in range(n)}
    stack, path = [0], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


class Rig:
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.batch = [t.to(DEV) for t in synth.make_inputs(CFG, B, L, LENGTHS, "randn", seed=1)]
        self.batch8 = [torch.cat([t, t], 0) for t in self.batch]
        teacher = torch.randn(B, L, C, generator=g).to(DEV)
        crf = LinearChainCRF(C).to(DEV)
        head = AuxiliaryHead(_model().m2f_config.cls_hidden, A).to(DEV)
        with torch.no_grad():
            crf.params.copy_((0.1 * torch.randn(crf.params.numel(), generator=g)).to(DEV))
        crf.params.requires_grad_(False)
        head.params.requires_grad_(False)
        aux = (head, torch.randint(0, A, (B, L), generator=g).to(DEV), 0.5)
        distill = {"teacher_logits": teacher, "distill": (0.3, 2.0)}
        self.kw = {"plain": {}, "distill": distill, "focal": {"focal_gamma": 2.0}, "distill+focal": dict(distill, focal_gamma=2.0),
                   "crf": {"crf": crf, "label_smoothing": 0.0}, "rdrop": {"rdrop": 0.5}, "supcon": {"supcon": (0.5, 0.2)},
                   "aux": {"aux": aux}, "aux+focal": {"aux": aux, "focal_gamma": 2.0}, "plain8": {}, "focal8": {"focal_gamma": 2.0}}
        # what each criterion gives a model that has run nothing else
        self.first = {name: self.step(_model(), name, False) for name in NINE + EIGHT}
        torch.cuda.synchronize()

    def step(self, model, name, use_graph):
        """One step of `model` under the criterion `name` from a zeroed tail -> the tail (loss, den, num, fourth float), on the device"""
        eng = model.engine()
        eng.ensure_grad()
        tail = eng.flat_grad_ext[eng.flat.numel(): eng.flat.numel() + 4]
        tail.zero_()
        model.train_step(*(self.batch8 if name in EIGHT else self.batch), use_graph=use_graph, **self.kw[name])
        return tail.clone()


@pytest.fixture(scope="module")
def rig():
    return Rig()


def test_the_criteria_differ_from_each_other(rig):
    """nine criteria, nine tails - otherwise 'the bits of its first visit' would prove little; a batch of 8 is the batch twice"""
    tails = {name: tuple(t.tolist()) for name, t in rig.first.items()}
    print(tails)
    assert all(torch.isfinite(t).all() for t in rig.first.values())
    assert len({tails[name] for name in NINE}) == 9
    assert all(tails[name][3] > 0.0 for name in ("supcon", "aux", "aux+focal")) and all(tails[name][3] == 0.0 for name in NINE[:6])
    assert tails["plain8"][1] == 2.0 * tails["plain"][1] and tails["focal8"][1] == 2.0 * tails["focal"][1]


def test_the_walk_takes_every_ordered_pair():
    walk = euler_walk(len(NINE))
    assert len(walk) == 73 and set(zip(walk, walk[1:])) == set(itertools.permutations(range(len(NINE)), 2))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_every_transition_gives_the_bits_of_the_first_visit(rig, use_graph):
    model = _model()
    names = [NINE[i] for i in euler_walk(len(NINE))]
    # R-Drop's plan of 8 dialogues: every ordered pair of what can hold it, then back among the plans of 4
    names += ["plain8", "rdrop", "focal8", "rdrop", "plain8", "focal8", "plain8", "aux+focal", "focal8", "plain"]
    seen = []
    for name in names:
        seen.append(rig.step(model, name, use_graph))
        seen.append(rig.step(model, name, use_graph))              # its criterion is held: no switch moves, a captured step replays
    got = torch.stack(seen).view(torch.int32).cpu()
    want = torch.stack([rig.first[name] for name in names for _ in range(2)]).view(torch.int32).cpu()
    wrong = [(i // 2, names[i // 2 - 1] if i >= 2 else None, names[i // 2]) for i in range(len(seen)) if not torch.equal(got[i], want[i])]
    assert not wrong, f"{len(wrong)} of {len(seen)} steps differ from their criterion's first visit; (step, from, to) of the first: {wrong[0]}"
    assert len(model.engine().plans) == 2                           # the plan of 4 dialogues and the plan of 8, nothing else was built


def test_eval_step_takes_a_trainable_crf_under_gradient_accumulation(rig):
    """An evaluation step writes no gradient: the block of a CRF that trains is an input there, whatever the training mode."""
    crf = LinearChainCRF(C).to(DEV)
    model, plain, acc = _model().eval(), DeviceScores(C, DEV), DeviceScores(C, DEV)
    assert crf.trainable
    model.eval_step(*rig.batch, plain, label_smoothing=0.0, crf=crf, use_graph=False)
    model.set_grad_accumulation(True)
    model.eval_step(*rig.batch, acc, label_smoothing=0.0, crf=crf, use_graph=False)
    assert torch.equal(plain.record, acc.record) and crf.params.grad is None
    with pytest.raises(ValueError, match="a trainable crf= does not combine with gradient accumulation"):
        model.train_step(*rig.batch, label_smoothing=0.0, crf=crf)
