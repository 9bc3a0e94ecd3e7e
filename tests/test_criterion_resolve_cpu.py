"""criterion.py on the host: every recorded answer of the step entry points to every combination of their criterion arguments
(tests/golden/criterion_refusals.json, recorded by tools/record_criterion_refusals.py on the commit before the rule table) replayed word
for word; the table against itself (every pair of kinds either combines or has a rule); and runtime.criterion_transition over every
ordered pair of the plan's reachable states, replayed against a model of the C side's exclusions."""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_criterion_refusals as rec  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import criterion  # noqa: E402
from mer_amd.runtime import criterion_transition  # noqa: E402


# ---- the recorded refusals --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with open(rec.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", rec.ENTRIES)
def test_every_recorded_outcome_is_unchanged(recorded, entry):
    rig = rec.Rig()
    cases = [c for c in rec.cases() if c[0] == entry]
    assert len(cases) == 864 and len(recorded["cases"]) == 3 * 864
    wrong = []
    for case in cases:
        want, got = recorded["messages"][recorded["cases"][rec.key(case)]], rig.outcome(case)
        if got != want:
            wrong.append((rec.key(case), want, got))
    assert not wrong, f"{len(wrong)} of {len(cases)} differ; the first: {wrong[0]}"
    assert rig.model._engine is None                                    # every one of them was answered before a device was asked for


def test_plain_is_a_short_cut():
    base = dict(num_classes=7, cls_hidden=64, mask_shape=(2, 5), device="cpu", label_smoothing=0.1, class_weights=None)
    assert criterion.resolve("step", **base) is criterion.PLAIN and criterion.PLAIN.kinds == ()
    assert criterion.resolve("step", **{**base, "accumulating": True, "data_parallel": True, "aux_label_smoothing": 5.0}) is criterion.PLAIN
    spec = criterion.resolve("step", **base, focal_gamma=2, teacher_logits=torch.zeros(2, 5, 7), distill=(0.5, 2))
    assert spec.kinds == ("distill", "focal") and (spec.distill, spec.gamma, spec.term_weight) == ((0.5, 2.0), 2.0, 0.0)
    with pytest.raises(ValueError, match="eval: rdrop is not an argument of an evaluation step"):
        criterion.resolve("eval", **base, evaluating=True, rdrop=1.0)


def test_every_pair_of_kinds_combines_or_has_a_rule():
    """One home per rule: a pair of kinds is in COMBINES, or exactly one of the two subjects names the other's argument(s) in RULES."""
    args = {"distill": ("teacher_logits", "distill"), "focal": ("focal_gamma",), "crf": ("crf",), "rdrop": ("rdrop",), "supcon": ("supcon",),
            "aux": ("aux",)}
    for a, b in itertools.combinations(criterion.KINDS, 2):
        sides = [s for s, o in ((a, b), (b, a)) if s in criterion.RULES and set(args[o]) <= {r[0] for r in criterion.RULES[s]}]
        assert (frozenset((a, b)) in criterion.COMBINES) != (len(sides) == 1), (a, b, sides)
    for subject, rules in criterion.RULES.items():                     # ... and no rule is written twice
        assert len({r[0] for r in rules}) == len(rules), subject
    for order in criterion.PRIORITY.values():
        assert set(order) <= set(criterion.RULES) and len(set(order)) == len(order)


# ---- the transition ---------------------------------------------------------------------------------------------------------------------
CRF, CRF2, AUX, AUX2 = (0x1000, None), (0x2000, 0x2100), (0x3000, None, 3), (0x3000, 0x3100, 3)
STATES = {"plain": {}, "distill": {"distill": True}, "focal": {"focal": True}, "distill+focal": {"distill": True, "focal": True},
          "crf": {"crf": CRF}, "rdrop": {"rdrop": True}, "supcon": {"supcon": True}, "aux": {"aux": AUX},
          "aux+focal": {"focal": True, "aux": AUX},
          # the same criteria over other buffers: a changed pointer is one call, not off-and-on
          "crf, other block": {"crf": CRF2}, "aux, now trainable": {"aux": AUX2}, "aux+focal, now trainable": {"focal": True, "aux": AUX2}}
ALLOWED = {frozenset(("distill", "focal")), frozenset(("aux", "focal"))}      # csrc/plan.hip exclusions[]: every other pair is refused


def _replay(held, calls):
    """The calls against a model of the C table: asking for a switch beside a held one it does not combine with is a refusal"""
    held = dict(held)
    for switch, value in calls:
        if value is None:
            assert switch in held, f"{switch} switched off twice"
            del held[switch]
            continue
        for other in held:
            assert other == switch or frozenset((switch, other)) in ALLOWED, f"{switch} asked while {other} is held"
        held[switch] = value
    return held


@pytest.mark.parametrize("a", list(STATES))
@pytest.mark.parametrize("b", list(STATES))
def test_transition_between_every_ordered_pair_of_states(a, b):
    held, wanted = dict(STATES[a]), dict(STATES[b])
    calls = criterion_transition(held, wanted)
    assert _replay(held, calls) == wanted
    offs = [i for i, (_, v) in enumerate(calls) if v is None]
    assert offs == list(range(len(offs)))                               # every off precedes every on
    assert len({s for s, _ in calls}) == len(calls)                     # one call per switch at the most
    assert {s for s, _ in calls} == {s for s in set(held) | set(wanted) if held.get(s) != wanted.get(s)}      # ... and none for what stays
    if a == b:
        assert calls == []
    assert held == STATES[a] and wanted == STATES[b]                    # pure: neither argument is written


def test_the_states_are_the_kinds_that_resolve_lets_through():
    assert criterion.COMBINES == ALLOWED
    assert {frozenset(s) for s in STATES.values()} == {frozenset()} | {frozenset((k,)) for k in criterion.KINDS} | set(criterion.COMBINES)
