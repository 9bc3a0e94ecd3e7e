"""The step's chain kernels store their results through buffer descriptors, write-through where that family's switch is on
(csrc/common.h: m2f_store_b128 / _b64 / _b32, M2F_WT_RING / M2F_WT_ROWS / M2F_WT_ATTN).  A store policy moves no value and no
address, so no bit may change and no byte outside a result may be touched:

  * ring GEMM epilogue, every form a step uses (64x64, 128x64, 128x128, and 256x128 bias-only): fp32 C and its bf16 shadow equal the
    register-staged 64x64 build's, bit for bit - for every term set {-, site} x {-, gate} x {-, residual} x {-, accumulate}, for the
    shadow-only form, at K = 64 (one k-tile) and K = 136 (a k-tail the range check zeroes), for a launch with interior and edge tiles
    (both store paths in one launch) and for a column-block result (ldc != N) inside a guard band that must stay untouched;
  * LayerNorm forward / backward, 16-byte path, d = 64 and 768, 8 rows, with and without a dropout site: outputs, shadows, statistics
    and partials equal the general path's bits; a guard row behind every buffer stays untouched;
  * one-tile dialogue attention forward / backward (B = 2, H = 2, L = 5 / 16, head dim 32 / 96): the bits recorded from the build in
    front of the change (tests/golden/chain_store_parent_bits.npz, made by make_chain_store_parent_bits.py), workspace around the
    results included;
  * visibility across launches - what a store policy could break: a tiny bf16 train plan (1 + 1 layers, B = 4, L = 16, dropout 0.4)
    stepped 20 times from the same restored rng state, eagerly and as graph replays, gives identical loss, logits and gradient bits
    every time and the same ones eager and replayed.  A launch that missed a predecessor's stores would read the previous step's
    (other dropout masks are NOT in play: the state is restored) or the guard values of the first step, and fail here.

Ring shapes: the ring forms are chosen by tile count (gemm_dispatch.hip: 80 tiles of 64x64, 150 of 128x64, 200 of 128x128, the
two-round rule for 256x128), so "one whole tile" is the smallest launch of whole tiles that reaches the form, at K = 64; the work per
launch stays a few MFLOP.  No tolerance anywhere.
"""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import make_chain_store_parent_bits as A  # noqa: E402
import make_rowwise_parent_bits as G  # noqa: E402
import mer_amd  # noqa: E402,F401

DEV = "cuda:0"
SENT = 7.5                                  # guard value (exact in bf16)

# form -> (BM, BN, rows, columns): the smallest whole-tile launch the chooser gives that form
RING = {"64x64": (64, 64, 640, 512), "128x64": (128, 64, 1280, 960), "128x128": (128, 128, 1280, 2560), "256x128": (256, 128, 2048, 2176)}
FORM_ID = {"64x64": 7, "128x64": 8, "128x128": 9, "256x128": 10}          # include/m2fnet_hip.h: M2F_FORM_RING_*


def _same(name, got, want):
    got, want = G.bits(got), G.bits(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = got != want
    n = int(diff.sum())
    assert n == 0, f"{name}: {n} of {got.size} elements differ (first at {tuple(int(i) for i in np.argwhere(diff)[0])})"


def _ring_pair(form, M, N, K, terms, shadow_only=False, guard=0, seed=0):
    """the same GEMM through the register-staged 64x64 build (tile = 64) and the ring form (automatic tile) -> [(ws, sh)] * 2.
    C is a block of a shadowed workspace, `guard` rows / columns of guard values around it (ldc = N + 2 guard)."""
    from mer_amd import functional as F, runtime
    from mer_amd.runtime import check, lib
    site, gate, res, acc = terms
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)          # noqa: E731
    a, b, bias = rn(M, K), rn(N, K), rn(N)
    kw = dict(bias=bias)
    if site:
        kw.update(drop_site=7, drop_p=0.4, rng=torch.tensor([11, 22, 3, 0], dtype=torch.int32, device=DEV))
    if gate:
        kw.update(gate=rn(M, N), gate_scale=1.25)
    if res:
        kw.update(res=rn(M, N))
    c0 = rn(M, N)
    shadows = [F._shadow16(t) for t in (a, b)]
    outs = []
    for tile in (64, 0):
        ws = torch.full((M + 2 * guard, N + 2 * guard), SENT, device=DEV)
        c = ws[guard:guard + M, guard:guard + N]
        c.copy_(c0 if acc else torch.full_like(c0, SENT))
        sh = ws.to(torch.bfloat16).contiguous()
        before = lib().m2f_gemm_ring_launches()
        check(lib().m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
        lib().m2f_set_shadow_only(1 if shadow_only else 0)
        try:
            F.gemm(a, b, F.NT, runtime.BF16, out=c, accumulate=bool(acc), tile=tile, shadows=(shadows[0], None, shadows[1], None), **kw)
            torch.cuda.synchronize()
        finally:
            lib().m2f_set_shadow_only(0)
            check(lib().m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
        took = lib().m2f_gemm_ring_launches() - before
        assert took == (1 if tile == 0 else 0), f"tile={tile}: {took} ring launches"
        if tile == 0:
            assert lib().m2f_gemm_last_form() & 0xFF == FORM_ID[form], f"form {lib().m2f_gemm_last_form() & 0xFF} ran, not the {form} ring form"
        outs.append((ws, sh))
    return outs


def _term_sets(form):
    if form == "256x128":                   # bias-only launches (the merged QKV in-projections)
        return [(0, 0, 0, 0)]
    return list(itertools.product((0, 1), repeat=4))


@pytest.mark.skipif(os.environ.get("M2F_RING", "1") == "0", reason="ring form switched off in the environment")
@pytest.mark.parametrize("K", [64, 136])
@pytest.mark.parametrize("form", sorted(RING))
def test_ring_epilogue_bits_every_term_set(form, K):
    _, _, M, N = RING[form]
    for n, terms in enumerate(_term_sets(form)):
        (ws0, sh0), (ws1, sh1) = _ring_pair(form, M, N, K, terms, seed=n)
        assert torch.isfinite(ws0).all()
        _same(f"{form} K={K} terms={terms} C", ws1, ws0)
        _same(f"{form} K={K} terms={terms} shadow", sh1, sh0)
    # the shadow-only form (no fp32 reader): the bf16 shadow is the result
    (ws0, sh0), (ws1, sh1) = _ring_pair(form, M, N, K, (0, 0, 0, 0), shadow_only=True, seed=99)
    _same(f"{form} K={K} shadow-only shadow", sh1, sh0)


@pytest.mark.skipif(os.environ.get("M2F_RING", "1") == "0", reason="ring form switched off in the environment")
@pytest.mark.parametrize("form", sorted(RING))
def test_ring_epilogue_interior_and_edge_tiles_in_one_launch(form):
    BM, BN, M, N = RING[form]
    terms = (0, 0, 0, 0) if form == "256x128" else (1, 1, 1, 1)
    (ws0, sh0), (ws1, sh1) = _ring_pair(form, M + 2, N + 8, 136, terms, seed=7)
    _same(f"{form} edge C", ws1, ws0)
    _same(f"{form} edge shadow", sh1, sh0)


@pytest.mark.skipif(os.environ.get("M2F_RING", "1") == "0", reason="ring form switched off in the environment")
@pytest.mark.parametrize("form", sorted(RING))
def test_ring_epilogue_column_block_leaves_the_guard_band_alone(form):
    BM, BN, M, N = RING[form]
    terms = (0, 0, 0, 0) if form == "256x128" else (0, 0, 1, 0)
    (ws0, sh0), (ws1, sh1) = _ring_pair(form, M, N, 64, terms, guard=8, seed=11)
    _same(f"{form} column block C", ws1, ws0)
    _same(f"{form} column block shadow", sh1, sh0)
    for name, t in (("C", ws1), ("shadow", sh1.float())):
        band = torch.ones_like(t, dtype=torch.bool)
        band[8:8 + M, 8:8 + N] = False
        assert bool((t[band] == SENT).all()), f"{form}: the guard band around {name} was written"
        assert not bool((t[~band] == SENT).all())


def _ln_run(d, site, general, T=8):
    """LayerNorm forward (residual, site) and backward (extra, masked second output at site + 4) over T rows; out / dx / dx_masked are
    blocks of one shadowed workspace, and every buffer has one guard row behind it.  general: every row buffer starts 4 bytes past a
    16-byte boundary (the general path: guarded element accesses)."""
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    o = 1 if general else 0
    i = {k: G.rand(*s, seed=300 + n, scale=sc) for n, (k, s, sc) in enumerate(
        [("x", (T, d), 3.0), ("res", (T, d), 1.0), ("dy", (T, d), 1.0), ("extra", (T, d), 1.0), ("g", (d,), 0.1), ("b", (d,), 0.1)])}

    def rows(t):
        flat = torch.zeros(T * d + 4)
        flat[o:o + T * d] = t.reshape(-1)
        return flat.to(DEV)[o:o + T * d].view(T, d)

    x, res, dy, extra = (rows(i[k]) for k in ("x", "res", "dy", "extra"))
    g, b = (1 + i["g"]).to(DEV), i["b"].to(DEV)
    blk = (T + 1) * d
    ws = torch.full((3 * blk + 4,), SENT, device=DEV)
    sh = ws.to(torch.bfloat16).contiguous()
    out, dx, dxm = (ws[o + n * blk:o + n * blk + T * d].view(T, d) for n in range(3))
    stats = torch.full((T + 1, 2), SENT, device=DEV)
    nblk = (T + 3) // 4
    partial = torch.full((nblk + 1, 2, d), SENT, device=DEV)
    dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    rng = G.rng_tensor()
    check(lib().m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        check(lib().m2f_layernorm_fwd_drop(T, d, d, ptr(x), ptr(g), ptr(b), ptr(res), ptr(out), ptr(stats), 1e-5,
                                           site, G.P_DROP if site else 0.0, ptr(rng) if site else None, stream_ptr()), "m2f_layernorm_fwd_drop")
        site2 = site + 4 if site else 0
        check(lib().m2f_layernorm_bwd_masked(T, d, d, ptr(x), ptr(g), ptr(stats), ptr(dy), ptr(extra), ptr(dx), ptr(dxm), ptr(partial),
                                             ptr(dg), ptr(db), site2, G.P_DROP if site2 else 0.0, ptr(rng) if site2 else None, stream_ptr()),
              "m2f_layernorm_bwd_masked")
        torch.cuda.synchronize()
    finally:
        check(lib().m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
    r = dict(stats=stats[:T], partial=partial[:nblk], dg=dg, db=db)
    guards = dict(stats=stats[T:], partial=partial[nblk:])
    for n, name in enumerate(("out", "dx", "dxm")):
        lo = o + n * blk
        r[name], r[name + "16"] = ws[lo:lo + T * d], sh[lo:lo + T * d]
        guards[name], guards[name + "16"] = ws[lo + T * d:lo + blk], sh[lo + T * d:lo + blk].float()
    return r, guards


@pytest.fixture(scope="module")
def ln_general():
    """the general path's results, computed once per (d, site)"""
    return {(d, site): _ln_run(d, site, True)[0] for d in (64, 768) for site in (0, 4)}


@pytest.mark.parametrize("site", [0, 4])
@pytest.mark.parametrize("d", [64, 768])
def test_layernorm_16_byte_path_bits_and_guard_rows(d, site, ln_general):
    fast, guards = _ln_run(d, site, False)
    want = ln_general[(d, site)]
    assert sorted(fast) == sorted(want)
    for k in sorted(fast):
        assert torch.isfinite(fast[k].float()).all(), k
        _same(f"ln d={d} site={site} {k}", fast[k], want[k])
    for k, t in guards.items():
        assert bool((t == SENT).all()), f"ln d={d} site={site}: the guard row behind {k} was written"


@pytest.fixture(scope="module")
def attn_recorded():
    with np.load(A.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", sorted(A.CASES))
def test_attention_one_tile_bits_are_the_recorded_ones(case, attn_recorded):
    got = A.compute(case)
    want = {k: v for k, v in attn_recorded.items() if k.split("/")[0] == case}
    assert sorted(got) == sorted(want) and got, (sorted(got), sorted(want))
    for k in sorted(got):
        diff = got[k] != want[k]
        assert got[k].shape == want[k].shape and not diff.any(), f"{k}: {int(diff.sum())} of {got[k].size} elements differ from the recorded bits"


def test_every_launch_sees_its_predecessors_stores_eager_and_replayed():
    import synth
    from mer_amd.model import M2FNet
    cfg = synth._cfg(64, 96, 64, 4, 4, 4, 1, 1, 1, dropout=0.4)          # 1 encoder layer per modality + 1 fusion layer
    B, L = 4, 16
    sd = synth.make_state_dict(cfg)
    batch = synth.make_inputs(cfg, B, L, [16, 9, 1, 12], "randn")
    torch.manual_seed(20261021)
    m = M2FNet(cfg, precision="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    eng = m.engine()
    dev = [t.cuda() for t in batch]
    m.train_step(*dev, use_graph=False)                 # builds the plan; its results are not compared
    plan = eng.plans[next(iter(eng.plans))]
    rng0 = eng.rng.clone()
    first = None
    for use_graph in (False, True):                     # (the captured step runs on the engine's own stream: M2FNet.train_step)
        for n in range(20):
            eng.rng.copy_(rng0)
            loss = m.train_step(*dev, use_graph=use_graph)
            torch.cuda.synchronize()
            got = dict(loss=G.bits(loss.reshape(-1)), logits=G.bits(plan.logits), grad=G.bits(eng.flat_grad))
            if first is None:
                first = got
                assert np.isfinite(loss.reshape(-1)[0].item()) and eng.flat_grad.abs().max().item() > 0
                continue
            for k in first:
                diff = got[k] != first[k]
                assert not diff.any(), f"{'replay' if use_graph else 'eager'} step {n}: {int(diff.sum())} of {got[k].size} {k} elements moved"
