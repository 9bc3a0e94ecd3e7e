"""DialogueStream.snapshot / restore / evict / fork: an interrupted stream against an uninterrupted one, bit for bit.

The model is the tiny_ragged fixture with S = 8 dialogues.  Every dialogue has its own inputs (utterance t of dialogue d is row [d, t] of
two fixed tensors), so a dialogue can sit in any slot of any stream and be compared with stream A, which runs the whole script without
an interruption: ragged steps and one chunked prefill (PHASE1), the interruption point, then another chunked prefill and more ragged
steps (PHASE2) - under past=None dialogue 0 reaches 38 utterances and dialogue 4 crosses a page boundary before the interruption, under
past=3 every ring wraps.  Every comparison is torch.equal."""
import contextlib
import functools
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import streaming  # noqa: E402
from mer_amd.streaming import StreamSnapshot  # noqa: E402
from test_streaming_model_gpu import _model  # noqa: E402

CFG = synth.CASES["tiny_ragged"][0]
S = 8
T_MAX = 48
ALL = [True] * S
# (kind, per-dialogue mask or counts)
PHASE1 = [("step", ALL), ("step", [d % 2 == 0 for d in range(S)]), ("prefill", [5, 0, 9, 2, 19, 7, 1, 4]), ("step", [d != 3 for d in range(S)])]
PHASE2 = [("prefill", [24, 3, 0, 10, 6, 1, 13, 2]), ("step", ALL), ("step", [d % 3 != 1 for d in range(S)]), ("step", [d != 5 for d in range(S)]),
          ("step", ALL), ("step", [d in (0, 2, 7) for d in range(S)]), ("step", ALL)]
MID = [8, 2, 12, 3, 22, 9, 4, 6]                 # utterances per dialogue at the interruption
END = [38, 9, 18, 18, 32, 14, 22, 13]
KINDS = {"dense": {}, "paged16": {"pages": 32, "page_rows": 16}, "paged32": {"pages": 20, "page_rows": 32}}
PARAMS = [(past, precision, graph) for past in (None, 3) for precision in ("fp32", "bf16") for graph in (True, False)]
IDS = [f"past{p}-{q}-{'graph' if g else 'eager'}" for p, q, g in PARAMS]


@functools.lru_cache(maxsize=None)
def _m(past, precision):
    with torch.inference_mode(False):           # (a model built under inference_mode cannot track its parameters' versions)
        return _model(CFG, past, precision)


@functools.lru_cache(maxsize=None)
def _inputs(seed=5):
    cfg = _m(None, "fp32").m2f_config
    g = torch.Generator().manual_seed(seed)
    return torch.randn(S, T_MAX, cfg.d_text, generator=g).cuda(), torch.randn(S, T_MAX, cfg.d_audio, generator=g).cuda()


def _open(streams, past, precision, graph, kind="dense", max_streams=S, capacity=None):
    kw = dict(KINDS[kind])
    if capacity is None and past is None:
        capacity = 64
    st = _m(past, precision).stream(max_streams, capacity=capacity, use_graph=graph, max_chunk=4, **kw)
    streams.append(st)
    return st


@contextlib.contextmanager
def _streams():
    streams = []
    try:
        with torch.inference_mode():
            yield streams
    finally:
        for st in streams:
            st.close()


class _Drive:
    """Feeds dialogues to a stream whatever slots they sit in: slot_of = {dialogue: slot}.  Results come back per DIALOGUE."""

    def __init__(self, st, slot_of=None):
        self.st = st
        self.slot_of = {d: d for d in range(S)} if slot_of is None else dict(slot_of)

    def step(self, mask):
        st, (XT, XA) = self.st, _inputs()
        n_slots = st.max_streams
        text, audio = torch.zeros(n_slots, XT.shape[2], device="cuda"), torch.zeros(n_slots, XA.shape[2], device="cuda")
        act = [False] * n_slots
        for d, s in self.slot_of.items():
            if mask[d]:
                act[s] = True
                text[s], audio[s] = XT[d, st.lengths[s]], XA[d, st.lengths[s]]
        out = st.step(text, audio, act)
        res = torch.zeros(S, out.shape[1], device="cuda")
        for d, s in self.slot_of.items():
            res[d] = out[s]
        return res

    def prefill(self, counts):
        st, (XT, XA) = self.st, _inputs()
        n_slots, n = st.max_streams, max(counts)
        text, audio = torch.zeros(n_slots, n, XT.shape[2], device="cuda"), torch.zeros(n_slots, n, XA.shape[2], device="cuda")
        cnt = [0] * n_slots
        for d, s in self.slot_of.items():
            c, at = counts[d], st.lengths[s]
            cnt[s] = c
            text[s, :c], audio[s, :c] = XT[d, at: at + c], XA[d, at: at + c]
        out = st.prefill(text, audio, cnt)
        res = torch.zeros(S, n, out.shape[2], device="cuda")
        for d, s in self.slot_of.items():
            res[d] = out[s]
        return res

    def run(self, ops):
        return [getattr(self, kind)(arg) for kind, arg in ops]

    def lengths(self):
        return {d: self.st.lengths[s] for d, s in self.slot_of.items()}


@functools.lru_cache(maxsize=None)
def _uninterrupted(past, precision, graph):
    """Stream A: (logits of PHASE1, logits of PHASE2), computed once per setting and never written to"""
    with _streams() as streams:
        a = _Drive(_open(streams, past, precision, graph))
        first = a.run(PHASE1)
        assert a.st.lengths == MID
        second = a.run(PHASE2)
        assert a.st.lengths == END and a.st.plan.len.cpu().tolist() == END
        assert all(torch.isfinite(x).all() for x in first + second)
        return first, second


def _same(got, want, dialogues, what=""):
    rows = torch.tensor(sorted(dialogues), device="cuda")
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[rows], w[rows]), f"op {i} differs from the uninterrupted stream {what}"


def _after_phase1(streams, past, precision, graph, kind="dense"):
    b = _Drive(_open(streams, past, precision, graph, kind))
    first = b.run(PHASE1)
    _same(first, _uninterrupted(past, precision, graph)[0], range(S))
    return b


def _check_slots(st, slot_of, lengths):
    want = [0] * st.max_streams
    for d, s in slot_of.items():
        want[s] = lengths[d]
    assert st.lengths == want and st.plan.len.cpu().tolist() == want


# ---- interrupted against uninterrupted -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [("dense", "dense"), ("dense", "paged16"), ("paged16", "dense"), ("paged16", "paged32")])
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_interrupted_equals_uninterrupted(past, precision, graph, src, dst):
    want = _uninterrupted(past, precision, graph)[1]
    with _streams() as streams:
        b = _after_phase1(streams, past, precision, graph, src)
        snap = b.st.snapshot()
        assert snap.lengths == MID and len(snap) == S and snap.data.is_cuda
        assert b.st.lengths == MID, "a snapshot leaves the stream as it was"
        # the same stream: snapshot, reset, restore
        b.st.reset()
        assert b.st.plan.len.cpu().tolist() == [0] * S
        b.st.restore(snap)
        _check_slots(b.st, b.slot_of, MID)
        assert torch.equal(b.st.snapshot().data.view(torch.int16), snap.data.view(torch.int16))
        # a separate stream of the same model, possibly of the other kind
        t = _Drive(_open(streams, past, precision, graph, dst))
        t.st.restore(snap)
        _check_slots(t.st, t.slot_of, MID)
        again = t.st.snapshot()
        assert again.lengths == snap.lengths and again.row_offsets == snap.row_offsets and again.signature == snap.signature
        assert torch.equal(again.data.view(torch.int16), snap.data.view(torch.int16)), "the format does not depend on dense / paged / page_rows"
        _same(b.run(PHASE2), want, range(S), f"({src}, same stream)")
        _same(t.run(PHASE2), want, range(S), f"({src} -> {dst})")
        for d in (b, t):
            _check_slots(d.st, d.slot_of, END)


# ---- other slots and other streams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_restore_under_a_permutation_into_fewer_slots_and_another_capacity(past, precision, graph):
    want = _uninterrupted(past, precision, graph)[1]
    with _streams() as streams:
        snap = _after_phase1(streams, past, precision, graph, "paged16").st.snapshot()
        perm = [3, 6, 0, 7, 1, 5, 2, 4]                          # dialogue d goes to slot perm[d]
        p = _Drive(_open(streams, past, precision, graph), {d: s for d, s in enumerate(perm)})
        p.st.restore(snap, perm)
        _check_slots(p.st, p.slot_of, MID)
        _same(p.run(PHASE2), want, range(S), "(permuted slots)")
        _check_slots(p.st, p.slot_of, END)

        few = _Drive(_open(streams, past, precision, graph, "paged16", max_streams=4), {1: 0, 5: 1, 6: 2})
        few.st.restore(snap.select([1, 5, 6]))
        _check_slots(few.st, few.slot_of, MID)
        _same(few.run(PHASE2), want, [1, 5, 6], "(select([1, 5, 6]) into max_streams = 4)")
        assert few.st.lengths[3] == 0

        if past is None:
            big = _Drive(_open(streams, past, precision, graph, capacity=128))
            assert big.st.capacity == 128 and snap.signature == big.st.signature
            big.st.restore(snap)
            _same(big.run(PHASE2), want, range(S), "(capacity 64 -> 128)")


# ---- through the host -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "paged16"])
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_evict_through_the_host_and_back(past, precision, graph, kind):
    want = _uninterrupted(past, precision, graph)[1]
    with _streams() as streams:
        b = _after_phase1(streams, past, precision, graph, kind)
        st = b.st
        paged = st.allocator is not None
        free0 = st.pages_free
        evicted = set(st.allocator.slot_pages[0] + st.allocator.slot_pages[3]) if paged else set()
        snap = st.evict([0, 3])
        assert snap.lengths == [MID[0], MID[3]] and not snap.data.is_cuda and snap.data.is_pinned()
        assert st.lengths[0] == 0 and st.lengths[3] == 0 and st.plan.len.cpu().tolist() == st.lengths
        if paged:
            assert len(evicted) == 2 and st.pages_free == free0 + len(evicted), "the evicted pages are free when evict returns"
        buf = io.BytesIO()
        torch.save(snap.state_dict(), buf)
        buf.seek(0)
        back = StreamSnapshot.from_state_dict(torch.load(buf, weights_only=True)).to("cuda")
        assert back.lengths == snap.lengths and back.signature == st.signature
        st.restore(back, [6, 7])                                # dialogues 6 and 7 end here; 0 and 3 resume in their slots
        if paged:
            assert evicted <= set(st.allocator.slot_pages[6] + st.allocator.slot_pages[7]), "the freed pages are handed out again"
        b.slot_of = {0: 6, 3: 7, 1: 1, 2: 2, 4: 4, 5: 5}
        _check_slots(st, b.slot_of, MID)
        _same(b.run(PHASE2), want, b.slot_of, f"({kind}, through the host)")
        _check_slots(st, b.slot_of, END)


# ---- bystanders, fork -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "paged16"])
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_bystanders_are_untouched_and_fork_copies_a_dialogue(past, precision, graph, kind):
    want = _uninterrupted(past, precision, graph)[1]
    with _streams() as streams:
        b = _after_phase1(streams, past, precision, graph, kind)
        b.st.restore(b.st.snapshot([5, 1]), [1, 5])             # dialogues 1 and 5 swap slots while the other six are live
        b.slot_of.update({5: 1, 1: 5})
        _check_slots(b.st, b.slot_of, MID)
        _same(b.run(PHASE2), want, range(S), f"({kind}, bystanders)")

        f = _after_phase1(streams, past, precision, graph, kind).st
        f.fork(2, 7)
        assert f.lengths[7] == f.lengths[2] == MID[2] and f.plan.len.cpu().tolist() == f.lengths
        XT, XA = _inputs()
        text, audio = XT[:, 40].clone(), XA[:, 40].clone()
        text[7], audio[7] = text[2], audio[2]
        out = f.step(text, audio)
        assert torch.equal(out[7], out[2]), "a fork gives its source's logits for its source's inputs"
        out = f.step(XT[:, 41], XA[:, 41])
        assert not torch.equal(out[7], out[2]), "... and goes its own way once the inputs differ"
        assert f.lengths[7] == f.lengths[2] == MID[2] + 2


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_refusals_leave_the_stream_as_it_was(past, precision, graph):
    with _streams() as streams:
        snap = _after_phase1(streams, past, precision, graph).st.snapshot()
        XT, XA = _inputs()
        small = []
        for _ in range(2):                                      # the target and its twin: a pool of two pages, both held
            st = _m(past, precision).stream(S, capacity=64 if past is None else None, use_graph=graph, pages=2, page_rows=16)
            streams.append(st)
            small.append(st)
            for i in range(2):
                st.step(XT[:, i], XA[:, i], [True, True] + [False] * 6)
        t, twin = small
        assert t.pages_free == 0
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[2\]") as err:
            t.restore(snap.select([2, 3, 5]), [0, 1, 2])        # three pages needed, the targets hold two, none is free
        assert "restore" in str(err.value)
        assert t.lengths == twin.lengths and t.pages_free == twin.pages_free == 0
        assert t.allocator.slot_pages == twin.allocator.slot_pages
        assert torch.equal(t.plan.table, twin.plan.table) and torch.equal(t.plan.len, twin.plan.len)
        act = [True, True] + [False] * 6
        assert torch.equal(t.step(XT[:, 2], XA[:, 2], act), twin.step(XT[:, 2], XA[:, 2], act)), "the target slots keep their dialogues"

        def refused(*args):                                     # a launch that fails AFTER the pages were decided: the host rolls back
            raise RuntimeError("launch refused")
        real, t.plan.scatter = t.plan.scatter, refused
        with pytest.raises(RuntimeError, match="launch refused"):
            t.restore(snap.select([2]), [0])
        t.plan.scatter = real
        assert t.lengths == twin.lengths and t.pages_free == twin.pages_free and t.allocator.slot_pages == twin.allocator.slot_pages
        assert torch.equal(t.allocator.table, twin.allocator.table) and torch.equal(t.plan.len, twin.plan.len)
        assert torch.equal(t.step(XT[:, 3], XA[:, 3], act), twin.step(XT[:, 3], XA[:, 3], act))
        assert torch.equal(t.plan.table, twin.plan.table)

        dense = _open(streams, past, precision, graph)
        other_past = _m(2 if past == 3 else 3, precision).stream(S, use_graph=graph)
        streams.append(other_past)
        other_prec = _m(past, "bf16" if precision == "fp32" else "fp32").stream(S, capacity=64 if past is None else None, use_graph=graph)
        streams.append(other_prec)
        for st in (other_past, other_prec):
            with pytest.raises(ValueError, match="snapshot was written under"):
                st.restore(snap)
            assert st.lengths == [0] * S
        if past is not None:
            ring6 = _open(streams, past, precision, graph, capacity=6)
            assert ring6.capacity == 6
            with pytest.raises(ValueError, match="snapshot was written under"):
                ring6.restore(snap)
        else:
            short = _open(streams, past, precision, graph, capacity=16)
            with pytest.raises(RuntimeError, match=r"slot\(s\) \[4\]"):
                short.restore(snap)                             # dialogue 4 holds 22 utterances
            assert short.lengths == [0] * S and short.plan.len.cpu().tolist() == [0] * S
        with pytest.raises(ValueError, match="twice"):
            dense.restore(snap.select([0, 1]), [3, 3])
        with pytest.raises(ValueError):
            dense.restore(snap.select([0, 1]), [3])
        with pytest.raises(ValueError):
            dense.restore(snap.select([0]), [S])
        with pytest.raises(ValueError):
            dense.restore(snap.cpu())
        with pytest.raises(ValueError):
            dense.snapshot([S])
        assert dense.lengths == [0] * S and dense.plan.len.cpu().tolist() == [0] * S


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "paged16"])
@pytest.mark.parametrize("past,precision,graph", PARAMS, ids=IDS)
def test_a_snapshot_holds_the_live_rows_and_nothing_else(past, precision, graph, kind):
    with _streams() as streams:
        b = _after_phase1(streams, past, precision, graph, kind)
        st = b.st
        bf16 = precision == "bf16"
        W = st.plan.snapshot_row_elems()
        assert W * (2 if bf16 else 4) == streaming.cache_bytes(st.plan.cfg, 1, 1, bf16)
        assert W == streaming.snapshot_row_elems(st.signature[0], bf16)
        assert sorted(st.signature[0]) == sorted(streaming.config_sites(st.plan.cfg))
        assert st.signature[1:] == (bf16, past, None if past is None else 4)
        snap = st.snapshot()
        rows = [min(n, st.capacity) for n in MID]
        assert snap.data.numel() == sum(rows) * W and snap.nbytes == sum(rows) * W * (2 if bf16 else 4)
        assert snap.data.dtype == (torch.bfloat16 if bf16 else torch.float32) and snap.lengths == MID
        assert snap.row_offsets == [sum(rows[:e]) for e in range(S)]
        assert torch.isfinite(snap.data.float()).all()
        st.reset([4])
        only4 = [d == 4 for d in range(S)]
        b.step(only4)
        b.step(only4)
        short = st.snapshot([4])
        assert short.lengths == [2] and short.data.numel() == 2 * W, "only the new dialogue's live rows"
        empty = st.snapshot([])
        assert len(empty) == 0 and empty.data.numel() == 0
        st.reset([1])
        one = st.snapshot([1, 4])
        assert one.lengths == [0, 2] and one.row_offsets == [0, 0] and torch.equal(one.data.view(torch.int16), short.data.view(torch.int16))
        st.restore(one, [4, 1])                                  # an empty entry resets its slot
        assert st.lengths[4] == 0 and st.lengths[1] == 2 and st.plan.len.cpu().tolist() == st.lengths
