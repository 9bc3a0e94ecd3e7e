"""The per-tensor tables of csrc/param_tables.hip on the device, at kernel level over bare flat buffers of a model layout: a step or
a norm issued tensor by tensor equals the one launch, a refused range touches nothing, the table cache hands every (configuration,
form, group map) its own entry - across two configurations and past its 32-map limit - and the table region behind the parameter
shadows holds the items layout.param_specs predicts.  Everything is compared bit for bit; nothing is timed."""
import ctypes

import numpy as np
import pytest
import torch

import param_tables_ref as ref
import synth
from mer_amd import layout, runtime

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
EMA_W = 0.25


def _cfg(name):
    return layout.M2FConfig.from_model_config(synth.CASES[name][0])


def _buffers(c, seed, shadows=False):
    """Seeded flat buffers of the layout: parameters, gradients, both moments (the second non-negative), the average."""
    total = ref.tensors(c)[1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = {k: torch.randn(total, device="cuda", generator=g) for k in ("p", "g", "m", "ema")}
    s["v"] = torch.rand(total, device="cuda", generator=g)
    if shadows:
        s["sh"] = runtime.param_shadow_buffer(c, "cuda")
    return s


def _clone(s):
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in s.items()}


def _same(a, b, what=""):
    torch.cuda.synchronize()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _table(groups=2):
    t = torch.zeros(runtime.ADAM_MAX_GROUPS, 8, dtype=torch.float32, device="cuda")
    runtime.adam_hyper_groups(t, [(1e-3 * (i + 1), (0.9, 0.999), 1e-8, 0.01, bool(i % 2), 3 + i) for i in range(groups)])
    return t


def _map(values):
    return (ctypes.c_int * len(values))(*values)


def _step(c, form, s, tg=None, table=None, first=0, end=-1, ema=True):
    avg = s["ema"] if ema else None
    if form == "single":
        runtime.adam_step_shadowed(c, s["p"], s["g"], s["m"], s["v"], s["sh"], 3, grad_scale=None, first=first, end=end, ema=avg,
                                   ema_w=EMA_W, **HYPER)
    else:
        runtime.adam_step_grouped(c, s["p"], s["g"], s["m"], s["v"], s.get("sh"), tg, table, first=first, end=end, ema=avg, ema_w=EMA_W)


def test_tiny_ragged_has_the_shapes_these_tests_need():
    ts = ref.tensors(_cfg("tiny_ragged"))[0]
    assert any(n > ref.SLICE for _, n, _ in ts)                                   # more than one slice
    assert any(n % 4 for _, n, _ in ts)                                           # a tail the 16-byte loads cannot take
    assert any(len(sh) == 2 and (sh[0] % 64 or sh[1] % 64) for _, _, sh in ts)    # a ragged 64 x 64 tile


@pytest.mark.parametrize("form", ["single", "grouped_shadowed", "grouped_slices"])
def test_a_step_issued_tensor_by_tensor_equals_the_one_launch(form):
    c = _cfg("tiny_ragged")
    ts, _ = ref.tensors(c)
    tg = _map([(-1 if i % 7 == 3 else i % 2) for i in range(len(ts))])            # two groups, some tensors in none
    table = _table()
    whole = _buffers(c, 5, shadows=form != "grouped_slices")
    parts = _clone(whole)
    if "sh" in whole:
        parts["sh"] = runtime.param_shadow_buffer(c, "cuda")
    _step(c, form, whole, tg, table)
    for i, (off, _, _) in enumerate(ts):
        _step(c, form, parts, tg, table, first=off, end=ts[i + 1][0] if i + 1 < len(ts) else -1)
    _same(whole, parts, form)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_norm_partials_of_per_tensor_calls_equal_the_whole_range(dtype):
    c = _cfg("tiny_ragged")
    ts, _ = ref.tensors(c)
    g = _buffers(c, 6)["g"].to(dtype)
    whole, parts = runtime.grad_norm_scratch(c, "cuda").fill_(-1.0), runtime.grad_norm_scratch(c, "cuda").fill_(-2.0)
    assert whole.numel() == ref.n_slices(c)
    runtime.grad_sumsq(c, g, whole)
    for i, (off, _, _) in enumerate(ts):
        runtime.grad_sumsq(c, g, parts, first=off, end=ts[i + 1][0] if i + 1 < len(ts) else -1)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts) and bool((whole >= 0).all())


def test_refused_ranges_touch_nothing():
    c = _cfg("tiny_ragged")
    n = len(ref.tensors(c)[0])
    s = _buffers(c, 7, shadows=True)
    s["scratch"] = runtime.grad_norm_scratch(c, "cuda").fill_(-1.0)
    tg, table = _map([0] * n), _table()
    before = _clone(s)
    flat = {k: v for k, v in s.items() if k != "sh"}
    calls = {
        "m2f_adam_step_shadowed_range": lambda f, e: _step(c, "single", s, first=f, end=e, ema=False),
        "m2f_adam_step_shadowed_range_ema": lambda f, e: _step(c, "single", s, first=f, end=e),
        "m2f_adam_step_grouped": lambda f, e: _step(c, "grouped", s, tg, table, first=f, end=e, ema=False),
        "m2f_adam_step_grouped (slices)": lambda f, e: _step(c, "grouped", flat, tg, table, first=f, end=e, ema=False),
        "m2f_adam_step_grouped_ema": lambda f, e: _step(c, "grouped", s, tg, table, first=f, end=e),
        "m2f_adam_step_grouped_ema (slices)": lambda f, e: _step(c, "grouped", flat, tg, table, first=f, end=e),
        "m2f_grad_sumsq": lambda f, e: runtime.grad_sumsq(c, s["g"], s["scratch"], first=f, end=e),
    }
    for entry, call in calls.items():
        for why, (first, end) in ref.bad_ranges(c).items():
            with pytest.raises(runtime.HipError) as err:
                call(first, end)
            assert entry.split(" ")[0] + ": " in str(err.value) and any(w in str(err.value) for w in ref.RANGE_WORDING), (entry, why)
    _same(before, s)


def _through_every_table(c, seed):
    """The norm's partials, the statistics record and a grouped step (slices form) of one configuration from one seeded state."""
    n = len(ref.tensors(c)[0])
    s = _buffers(c, seed)
    scratch = runtime.grad_norm_scratch(c, "cuda")
    runtime.grad_sumsq(c, s["g"], scratch)
    st_scratch, record = runtime.tensor_stats_buffers(c, 16, "cuda")
    runtime.tensor_stats(c, s["g"], st_scratch, record, 16)
    _step(c, "grouped", s, _map([i % 3 - 1 for i in range(n)]), _table())
    return dict(s, scratch=scratch, record=record)


def test_two_configurations_alternate_through_the_cache():
    a, b = _cfg("tiny_ragged"), _cfg("c2_slice")
    a1, a2 = _through_every_table(a, 8), _through_every_table(a, 8)                # nothing else in between
    b1 = _through_every_table(b, 9)
    a3 = _through_every_table(a, 8)
    b2 = _through_every_table(b, 9)
    _same(a1, a2, "tiny_ragged twice")
    _same(a1, a3, "tiny_ragged after c2_slice")
    _same(b1, b2, "c2_slice after tiny_ragged")


@pytest.mark.parametrize("form", ["grouped_shadowed", "grouped_slices"])
def test_more_group_maps_than_the_cache_keeps(form):
    c = _cfg("tiny_ragged")
    n = len(ref.tensors(c)[0])
    table = _table()
    start = _buffers(c, 10, shadows=form == "grouped_shadowed")
    maps = [_map([(-1 if i == k else i % 2) for i in range(n)]) for k in range(34)]          # 34 distinct maps: two more than are kept

    def run(tg):
        s = _clone(start)
        _step(c, form, s, tg, table)
        return _clone(s)

    first = run(maps[0])
    for tg in maps[1:]:
        run(tg)
    _same(first, run(maps[0]), "the first map again, after its entry was dropped")


@pytest.mark.parametrize("form", ["grouped_shadowed", "grouped_slices"])
def test_a_map_and_its_complement_never_share_an_entry(form):
    c = _cfg("tiny_ragged")
    ts, total = ref.tensors(c)
    even = [0 if i % 2 == 0 else -1 for i in range(len(ts))]
    odd = [-1 if i % 2 == 0 else 0 for i in range(len(ts))]
    table = _table()
    start = _buffers(c, 11, shadows=form == "grouped_shadowed")
    for owners in (even, odd, even, odd):
        s = _clone(start)
        _step(c, form, s, _map(owners), table)
        torch.cuda.synchronize()
        unowned = torch.zeros(total, dtype=torch.bool, device="cuda")
        for (off, numel, _), g in zip(ts, owners):
            if g < 0:
                unowned[off: off + numel] = True
        for k in ("p", "m", "v", "ema"):
            assert torch.equal(s[k][unowned], start[k][unowned]), (form, k)
            assert not torch.equal(s[k][~unowned], start[k][~unowned]), (form, k)


@pytest.mark.parametrize("name", ["tiny_ragged", "c2_slice"])
def test_the_table_region_behind_the_shadows(name):
    c = _cfg(name)
    sh = runtime.param_shadow_buffer(c, "cuda")
    torch.cuda.synchronize()
    region = sh[sh.numel() - ref.TABLE_BYTES // 2:].cpu().numpy().tobytes()
    want, prefix = ref.items(c)
    n = len(want)
    got = (ref.AdamItemC * n).from_buffer_copy(region)
    assert [(it.off, it.rows, it.cols, it.tiles_c, it.tile_begin) for it in got] == want
    at = n * ctypes.sizeof(ref.AdamItemC)
    assert np.frombuffer(region, dtype=np.int32, count=n + 1, offset=at).tolist() == prefix
    assert not any(region[at + 4 * (n + 1):])                                     # the rest of the region stays zero
