"""The plan's criterion switches (m2f_plan_distill, m2f_plan_focal, m2f_plan_rdrop, m2f_plan_crf) against each other, and a trainable
CRF block against gradient accumulation and the split step: csrc/plan.hip keeps these rules as rows of its exclusions[] table.  Every
ordered pair of the four switches - hold one, ask for the other - and the three trainable-CRF cases run on one small train plan,
through the C entry points themselves (the Python wrappers keep host mirrors and would not ask twice).  Distillation and focal
combine, in either order; every other pair is refused with the message below, word for word - the strings are the ones the entry
points printed when each carried its own `if` lines, not copies of the table.  A refused call leaves the plan as it was: the next
step gives the bits of the loss the step before the call gave."""
import itertools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.runtime import lib, ptr  # noqa: E402

DEV = "cuda"
CFG = synth._cfg(48, 64, 64, 4, 4, 4, 2, 2, 2, ncls=7)          # dropout 0 (tests/test_rdrop_model_gpu.py's)
C = 7
SWITCHES = ("distill", "focal", "rdrop", "crf")
# (asked, held) -> what the entry point says
REFUSALS = {
    ("distill", "crf"): "m2f_plan_distill: the CRF criterion is on (m2f_plan_crf): it has no distillation form",
    ("distill", "rdrop"): "m2f_plan_distill: the R-Drop criterion is on (m2f_plan_rdrop): it has no distillation form",
    ("focal", "crf"): "m2f_plan_focal: the CRF criterion is on (m2f_plan_crf): it has no focal form",
    ("focal", "rdrop"): "m2f_plan_focal: the R-Drop criterion is on (m2f_plan_rdrop): it has no focal form",
    ("rdrop", "distill"): "m2f_plan_rdrop: the distillation criterion is on (m2f_plan_distill): the R-Drop criterion has no distillation form",
    ("rdrop", "focal"): "m2f_plan_rdrop: the focal criterion is on (m2f_plan_focal): the R-Drop criterion has no focal form",
    ("rdrop", "crf"): "m2f_plan_rdrop: the CRF criterion is on (m2f_plan_crf): it has no R-Drop form",
    ("crf", "focal"): "m2f_plan_crf: the focal criterion is on (m2f_plan_focal): the CRF criterion has no focal form",
    ("crf", "distill"): "m2f_plan_crf: the distillation criterion is on (m2f_plan_distill): the CRF criterion has no distillation form",
    ("crf", "rdrop"): "m2f_plan_crf: the R-Drop criterion is on (m2f_plan_rdrop): the CRF criterion has no R-Drop form",
}
ALLOWED = {("focal", "distill"), ("distill", "focal")}
TRAINABLE_CRF = {
    # name: (held, asked, message)
    "accumulate_while_training_a_crf": ("crf_train", "accumulate",
                                        "m2f_plan_accumulate_grads: the plan trains a CRF block (m2f_plan_crf with param_grad): its gradient is "
                                        "normalised by one batch's den; freeze it (param_grad NULL) first"),
    "trainable_crf_while_accumulating": ("accumulate", "crf_train",
                                         "m2f_plan_crf: the plan accumulates gradients (m2f_plan_accumulate_grads): a trainable CRF block "
                                         "(param_grad) would need the group's den; pass param_grad NULL (frozen)"),
    "split_step_while_training_a_crf": ("crf_train", "split",
                                        "m2f_step_part: the plan trains a CRF block (m2f_plan_crf with param_grad): the split step belongs to the "
                                        "data-parallel reducer, which does not reduce that gradient; freeze it (param_grad NULL)"),
}


class Rig:
    """One train plan with a batch in it, every criterion's inputs filled, and the C entry points by name"""

    def __init__(self):
        B, L, lengths = 4, 6, [6, 6, 5, 6]
        m = M2FNet(CFG, precision="fp32")
        m.load_state_dict(synth.make_state_dict(CFG))
        self.model = m.to(DEV).train()
        batch = [t.to(DEV) for t in synth.make_inputs(CFG, B, L, lengths, "randn", seed=1)]
        self.model.train_step(*batch, use_graph=False)
        self.plan = self.model.engine().plans[next(reversed(self.model.engine().plans))]
        p = self.plan
        g = torch.Generator().manual_seed(5)
        p.set_teacher(torch.randn(B, L, C, generator=g).to(DEV))
        p.set_distill_hyper(0.3, 2.0)
        p.set_focal_gamma(2.0)
        p.partner_in.copy_(torch.arange(p.T, dtype=torch.int32).view(-1, 2).flip(1).reshape(-1).to(DEV))     # rows 2i <-> 2i + 1
        p.rdrop_alpha.fill_(0.5)
        self.crf_params = (0.1 * torch.randn(C * C + 2 * C, generator=g)).to(DEV)
        self.crf_grad = torch.zeros_like(self.crf_params)
        torch.cuda.synchronize()

    def ask(self, what, on=True):
        """-> (return code, the library's last error) of the C entry point behind `what`"""
        h = self.plan._h()
        if what == "distill":
            rc = lib().m2f_plan_distill(h, int(on))
        elif what == "focal":
            rc = lib().m2f_plan_focal(h, int(on))
        elif what == "rdrop":
            rc = lib().m2f_plan_rdrop(h, int(on))
        elif what in ("crf", "crf_train"):
            rc = lib().m2f_plan_crf(h, ptr(self.crf_params) if on else None, ptr(self.crf_grad) if on and what == "crf_train" else None)
        elif what == "accumulate":
            rc = lib().m2f_plan_accumulate_grads(h, int(on))
        elif what == "split":
            rc = lib().m2f_step_part(h, 0, 0.1, 0, 1, 0, torch.cuda.current_stream().cuda_stream)
        else:
            raise ValueError(what)
        return rc, lib().m2f_last_error().decode()

    def all_off(self):
        for what in SWITCHES + ("accumulate",):
            assert self.ask(what, on=False)[0] == 0

    def loss(self):
        """(loss, den, num, kl) of one eager step on the rig's batch, from a zeroed tail (the accumulate form adds to den, num and kl)"""
        self.plan.loss.zero_()
        return self.plan.step(use_graph=False).clone()


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture
def plain_rig(rig):
    rig.all_off()
    yield rig
    rig.all_off()


def _held_then_asked(rig, held, asked, message):
    rc, said = rig.ask(held)
    assert rc == 0, said
    before = rig.loss()
    assert torch.isfinite(before).all()
    rc, said = rig.ask(asked)
    if message is None:
        assert rc == 0, said
        both = rig.loss()
        assert torch.isfinite(both).all() and not torch.equal(both[0], before[0])      # the combined form is another criterion
        return
    assert rc != 0 and said == message
    after = rig.loss()
    assert torch.equal(after.view(torch.int32), before.view(torch.int32)), (before.tolist(), after.tolist())


@pytest.mark.parametrize("held,asked", list(itertools.permutations(SWITCHES, 2)), ids=lambda s: s)
def test_every_ordered_pair_of_the_criterion_switches(plain_rig, held, asked):
    assert ((asked, held) in REFUSALS) != ((asked, held) in ALLOWED)
    _held_then_asked(plain_rig, held, asked, REFUSALS.get((asked, held)))


@pytest.mark.parametrize("name", list(TRAINABLE_CRF))
def test_a_trainable_crf_block_against_accumulation_and_the_split_step(plain_rig, name):
    held, asked, message = TRAINABLE_CRF[name]
    _held_then_asked(plain_rig, held, asked, message)


def test_the_held_criteria_differ_from_each_other(plain_rig):
    """the rig's inputs make every switch count: five criteria, five tails (loss, den, num, kl) - otherwise 'the same loss as before' would
    prove little.  (The synthetic model's logits are nearly uniform, so the R-Drop term can vanish in the loss's fp32; its KL share, the
    tail's fourth float, cannot.)"""
    tails = [tuple(plain_rig.loss().tolist())]
    for what in SWITCHES:
        assert plain_rig.ask(what)[0] == 0
        tails.append(tuple(plain_rig.loss().tolist()))
        assert plain_rig.ask(what, on=False)[0] == 0
    assert len(set(tails)) == 5 and tails[3][3] > 0.0 and tails[0][3] == 0.0, tails
