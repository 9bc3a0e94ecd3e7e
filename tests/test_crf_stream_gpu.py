"""The CRF's forward filter on a stream (``model.stream(..., crf=module)``): ``crf_posterior()`` after steps, prefill and ``run`` against
the float64 filter on the returned logits (1e-5), dense and paged streams, ``past`` None and 3; ``reset``; snapshots / restore / evict /
fork bit for bit; the refusals; and logits that are ``torch.equal`` to those of a stream without ``crf=``.
Every comparison prints its figures before it asserts (-s)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_cases as cases  # noqa: E402
import crf_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd.crf import LinearChainCRF  # noqa: E402
from mer_amd.streaming import StreamSnapshot  # noqa: E402
from test_streaming_model_gpu import _model  # noqa: E402

CFG = synth.CASES["tiny_ragged"][0]
C = 7
S = 6
KINDS = {"dense": {}, "paged16": {"pages": 24, "page_rows": 16}}
# the script: ragged steps, one chunked prefill, more steps
SCRIPT = [("step", [True] * S), ("step", [d % 2 == 0 for d in range(S)]), ("prefill", [5, 0, 9, 2, 1, 7]), ("step", [d != 3 for d in range(S)]),
          ("step", [True] * S)]


@functools.lru_cache(maxsize=None)
def _m(past):
    with torch.inference_mode(False):
        return _model(CFG, past, "fp32")


def _crf(seed=21):
    crf = LinearChainCRF(C).cuda()
    with torch.no_grad():
        crf.params.copy_(cases.params_block(C, seed, 0.7))
    crf.params.requires_grad_(False)
    return crf


@functools.lru_cache(maxsize=None)
def _inputs():
    cfg = _m(None).m2f_config
    g = torch.Generator().manual_seed(5)
    return torch.randn(S, 40, cfg.d_text, generator=g).cuda(), torch.randn(S, 40, cfg.d_audio, generator=g).cuda()


def _open(past, kind, crf, graph=True):
    return _m(past).stream(S, capacity=64 if past is None else None, use_graph=graph, max_chunk=4, crf=crf, **KINDS[kind])


def _play(st, script, at, rows=None):
    """Feeds the script from per-dialogue positions `at` (updated); returns the logits of every call and, per slot, the logit rows it took."""
    XT, XA = _inputs()
    outs = []
    for what, arg in script:
        if what == "step":
            text = torch.stack([XT[d, at[d]] for d in range(S)])
            audio = torch.stack([XA[d, at[d]] for d in range(S)])
            out = st.step(text, audio, arg)
            for d in range(S):
                if arg[d]:
                    if rows is not None:
                        rows[d].append(out[d].cpu())
                    at[d] += 1
        else:
            n = max(arg)
            text = torch.stack([XT[d, at[d]: at[d] + n] for d in range(S)])
            audio = torch.stack([XA[d, at[d]: at[d] + n] for d in range(S)])
            out = st.prefill(text, audio, arg)
            for d in range(S):
                if rows is not None:
                    rows[d].extend(out[d, : arg[d]].cpu())
                at[d] += arg[d]
        outs.append(out.clone())
    return outs


def _against_filter(phi, rows, params, what):
    worst = 0.0
    for d in range(S):
        if not rows[d]:
            assert (phi[d] == 0).all()
            continue
        want = ref.filter_rows(torch.stack(rows[d]), params.cpu())[-1]
        worst = max(worst, float((phi[d].double().cpu() - want).abs().max()))
        assert abs(float(phi[d].exp().sum()) - 1.0) <= 1e-5
    print(f"{what}: max abs err of crf_posterior against the float64 filter on the returned logits {worst:.3g}")
    assert worst <= 1e-5


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("past", [None, 3])
def test_posterior_follows_the_filter_and_the_logits_are_untouched(past, kind, graph):
    crf = _crf()
    st, plain = _open(past, kind, crf, graph), _open(past, kind, None, graph)
    try:
        at, rows = [0] * S, [[] for _ in range(S)]
        a = _play(st, SCRIPT, at, rows)
        b = _play(plain, SCRIPT, [0] * S)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "crf= must not change a logit"
        _against_filter(st.crf_posterior(), rows, crf.params.detach(), f"past {past} {kind} graph {graph}")
        # reset of some slots clears their state; they start from `start` again
        st.reset([1, 4])
        phi = st.crf_posterior()
        assert (phi[[1, 4]] == 0).all() and (phi[[0, 2, 3, 5]] != 0).any(1).all()
        for d in (1, 4):
            at[d], rows[d] = 0, []
        _play(st, [("step", [True] * S)], at, rows)
        _against_filter(st.crf_posterior(), rows, crf.params.detach(), "after reset([1, 4]) and a step")
        st.reset()
        assert (st.crf_posterior() == 0).all()
        with pytest.raises(RuntimeError, match="without a CRF"):
            plain.crf_posterior()
    finally:
        st.close()
        plain.close()


@pytest.mark.parametrize("past", [None, 3])
def test_run_leaves_the_posterior_of_every_dialogues_last_utterance(past):
    crf = _crf()
    XT, XA = _inputs()
    lengths = [12, 3, 7, 1, 9, 12]
    mask = torch.ones(S, 12, dtype=torch.bool)
    for d, n in enumerate(lengths):
        mask[d, :n] = False
    st, plain = _open(past, "dense", crf), _open(past, "dense", None)
    try:
        out = st.run(XT[:, :12], XA[:, :12], mask.cuda())
        assert torch.equal(out, plain.run(XT[:, :12], XA[:, :12], mask.cuda()))
        rows = [list(out[d, :n].cpu()) for d, n in enumerate(lengths)]
        _against_filter(st.crf_posterior(), rows, crf.params.detach(), f"run, past {past}")
    finally:
        st.close()
        plain.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_snapshots_carry_the_filter_state(kind):
    crf = _crf()
    a, b, plain = _open(None, kind, crf), _open(None, kind, crf), _open(None, kind, None)
    try:
        at_a, at_b = [0] * S, [0] * S
        _play(a, SCRIPT, at_a)
        _play(b, SCRIPT, at_b)
        snap = b.snapshot()
        assert snap.crf is not None and torch.equal(snap.crf, b.crf_posterior())
        # through select / cpu / to / state_dict
        moved = StreamSnapshot.from_state_dict(snap.cpu().state_dict()).to("cuda")
        assert torch.equal(moved.crf, snap.crf) and torch.equal(snap.select([4, 1]).crf, snap.crf[[4, 1]])
        assert "crf" in snap.state_dict() and "crf" not in plain.snapshot().state_dict()
        b.reset()
        b.restore(moved)
        assert torch.equal(b.crf_posterior(), a.crf_posterior())
        # evict two slots, run the others on, bring them back: the uninterrupted stream's bits
        ev = b.evict([2, 5])
        assert (b.crf_posterior()[[2, 5]] == 0).all()
        b.restore(ev.to("cuda"), [2, 5])                  # (an evicted snapshot lives in pinned host memory: the K / V rows need the device)
        tail = [("step", [True] * S), ("prefill", [2, 4, 0, 1, 3, 2]), ("step", [True] * S)]
        oa, ob = _play(a, tail, at_a), _play(b, tail, at_b)
        assert all(torch.equal(x, y) for x, y in zip(oa, ob)) and torch.equal(a.crf_posterior(), b.crf_posterior())
        # fork: slot 3 becomes a copy of slot 0
        b.fork(0, 3)
        assert torch.equal(b.crf_posterior()[3], b.crf_posterior()[0]) and b.lengths[3] == b.lengths[0]
        # a snapshot with the state into a stream without it, and the reverse
        with pytest.raises(RuntimeError, match="carries a CRF filter state"):
            plain.restore(snap)
        _play(plain, SCRIPT, [0] * S)
        with pytest.raises(RuntimeError, match="carries no CRF filter state"):
            b.restore(plain.snapshot())
    finally:
        for st in (a, b, plain):
            st.close()


def test_refusals():
    m = _m(None)
    with pytest.raises(ValueError, match="classes"):
        m.stream(S, capacity=64, crf=LinearChainCRF(5).cuda())
    with pytest.raises(ValueError, match="LinearChainCRF"):
        m.stream(S, capacity=64, crf=torch.zeros(63))
    with pytest.raises(ValueError, match="move the module"):
        m.stream(S, capacity=64, crf=LinearChainCRF(C))


def test_stream_switch_refusals_at_the_c_entry():
    """m2f_plan_stream_crf by hand: a plan that is no stream plan, params without phi, misaligned params."""
    from mer_amd import runtime
    from test_crf_model_gpu import _batch, _last_plan, _model as _train_model
    lib = runtime.lib()
    crf = _crf()
    phi = torch.zeros(S, C, device="cuda")
    m = _train_model()
    m.train_step(*_batch(6, 12, 1), use_graph=False)
    for args, msg in (((_last_plan(m)._h(), crf.params.data_ptr(), phi.data_ptr()), "needs a stream or chunk plan"),):
        assert lib.m2f_plan_stream_crf(*args) != 0 and msg in lib.m2f_last_error().decode()
    st = _open(None, "dense", None)
    try:
        h = st.plan._h()
        assert lib.m2f_plan_stream_crf(h, crf.params.data_ptr(), None) != 0 and "come together" in lib.m2f_last_error().decode()
        assert lib.m2f_plan_stream_crf(h, None, phi.data_ptr()) != 0 and "come together" in lib.m2f_last_error().decode()
        assert lib.m2f_plan_stream_crf(h, crf.params.data_ptr() + 4, phi.data_ptr()) != 0 and "16-byte aligned" in lib.m2f_last_error().decode()
        assert lib.m2f_plan_stream_crf(h, None, None) == 0                                  # off while off: nothing to do
        assert lib.m2f_plan_stream_crf(h, crf.params.data_ptr(), phi.data_ptr()) == 0       # ... and on, then off again
        assert lib.m2f_plan_stream_crf(h, None, None) == 0
    finally:
        st.close()
