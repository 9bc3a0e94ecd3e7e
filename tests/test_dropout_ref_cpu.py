"""The host replica of the dropout masks (tests/golden/dropout_ref.py) against a second implementation written here on plain
Python ints (`& 0xffffffff` after every operation, from csrc/common.h), its statistics, and the site order of two configs."""
import math
import random

import numpy as np
import pytest

import synth
import dropout_ref as R

M = 0xFFFFFFFF


def _mix(x):
    x &= M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M
    x ^= x >> 15
    x = (x * 0x846CA68B) & M
    x ^= x >> 16
    return x


def _key(st, site):
    k = _mix(st[0] ^ 0x9E3779B9)
    k = _mix(k ^ st[1])
    k = _mix((k + st[2] * 0x85EBCA6B) & M)
    k = _mix(k ^ ((st[3] + site * 0xC2B2AE35) & M))
    return k


def _keep(key, idx, thresh):
    h = _mix((idx * 0x9E3779B1 + key) & M)
    h = _mix(h ^ (key >> 7) ^ 0x68E31DA4)
    return h >= thresh


def _values():
    rnd = random.Random(5)
    return [0, 1, M] + [rnd.getrandbits(32) for _ in range(300)]


def test_mix32_matches_scalar_implementation():
    v = _values()
    got = R.mix32(np.array(v, dtype=np.uint32))
    assert got.dtype == np.uint32
    assert got.tolist() == [_mix(x) for x in v]
    assert int(R.mix32(np.uint32(M))) == _mix(M)


def test_site_key_and_keep_match_scalar_implementation():
    v = _values()
    rnd = random.Random(6)
    states = [[0, 0, 0, 0], [M, M, M, M], [1, 0, M, 0], [123, 456, 7, 0]] + [[rnd.getrandbits(32) for _ in range(4)] for _ in range(40)]
    for i, st in enumerate(states):
        for site in (0, 1, 2, 17, M, rnd.getrandbits(32)):
            k = int(R.site_key(st, site))
            assert k == _key(st, site), (st, site)
        thresh = [0, 1, M, R.thresh_scale(0.3)[0]][i % 4]
        got = R.keep(k, np.array(v, dtype=np.uint32), thresh)
        assert got.tolist() == [_keep(k, x, thresh) for x in v]


def test_thresh_scale_rule():
    assert R.thresh_scale(0.0) == (0, 1.0)
    assert R.thresh_scale(0.5) == (1 << 31, 2.0)
    t, s = R.thresh_scale(0.3)
    assert t == math.floor(float(np.float32(0.3)) * 2.0 ** 32) and s == float(np.float32(1) / (np.float32(1) - np.float32(0.3)))
    assert R.thresh_scale(1.0)[0] == M                                        # clamped
    assert R.keep(R.site_key([9, 8, 3, 0], 4), np.arange(1 << 12, dtype=np.uint32), 0).all(), "thresh = 0 keeps everything"


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_keep_rate_is_binomial(p):
    n = 1 << 17
    sd = math.sqrt(p * (1 - p) / n)
    for site in (1, 2, 17):
        rate = R.rows_mask([123, 456, 7, 0], site, p, 256, n // 256).mean()
        assert abs(rate - (1 - p)) <= 4 * sd, (site, rate)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_sites_and_steps_draw_independent_masks(p):
    n = 1 << 17
    q = 2 * p * (1 - p)
    sd = math.sqrt(q * (1 - q) / n)
    base = R.rows_mask([123, 456, 7, 0], 5, p, 512, n // 512)
    for other in (R.rows_mask([123, 456, 7, 0], 6, p, 512, n // 512),          # the next site
                  R.rows_mask([123, 456, 8, 0], 5, p, 512, n // 512),          # the next step
                  R.rows_mask([123, 456, 7, 1], 5, p, 512, n // 512)):         # the step counter's high word
        assert abs((base != other).mean() - q) <= 4 * sd


def test_index_rules():
    st, p = [11, 22, 3, 0], 0.4
    thresh = R.thresh_scale(p)[0]
    m = R.rows_mask(st, 7, p, 9, 50)
    k = int(R.site_key(st, 7))
    assert m.shape == (9, 50) and all(m[r, c] == _keep(k, r * 50 + c, thresh) for r, c in [(0, 0), (3, 49), (8, 7)])
    a = R.attn_mask(st, 7, p, 2, 3, 16)
    assert a.shape == (2, 3, 16, 16)
    assert all(a[b, h, i, j] == _keep(k, ((b * 3 + h) * 16 + i) * 16 + j, thresh) for b, h, i, j in [(0, 0, 0, 0), (1, 2, 15, 3), (1, 0, 4, 9)])
    # the index wraps in 32 bits, as the kernels' uint32 arithmetic does
    wide = R.keep(k, R.rows_index([69999], 65536), thresh)[0, :4]
    assert wide.tolist() == [_keep(k, (69999 * 65536 + c) & M, thresh) for c in range(4)]


@pytest.mark.parametrize("name,count", [
    ("tiny_shared_norm", 2 * 1 * 4 + 2 + 3 * 2 * 4 + 2 + 1 * 2 + 1),           # 2 audio stacks x 1 layer, 3 text stacks x 2 layers, 1 fusion layer
    ("tiny_no_fam", 4 + 2 + 4 + 2 + 1)])
def test_site_map_order(name, count):
    cfg = synth.CASES[name][0]
    sites = R.site_map(cfg)
    assert len(sites) == count
    assert list(sites.values()) == list(range(1, count + 1)), "sites are handed out from 1, no duplicates"
    names = list(sites)
    assert names[:4] == ["audio_encoders.0.layers.0." + w for w in ("attn", "dropout1", "ff", "dropout2")]
    assert names[-1] == "classifier"
    a_pre, a_post = names.index("audio.pre_proj"), names.index("audio.post_proj")
    assert a_post == a_pre + 1 and names[a_post + 1].startswith("text_encoders.0.layers.0.")
    assert names[a_pre - 1] == f"audio_encoders.{cfg['AUDIO']['n_transformers'] - 1}.layers.{cfg['AUDIO']['n_encoder_layers'] - 1}.dropout2"
    if name == "tiny_shared_norm":
        assert names[-3:-1] == ["fusion_layers.0.attn", "fusion_layers.0.out"]
    else:
        assert names[-2] == "text.post_proj"


def _hook(cfg, B, L, p, state=(5, 6, 1, 0)):
    """PlanMasks of a padded plan of exactly the batch's shape."""
    rows = np.arange(B)[:, None] * L + np.arange(L)[None, :]
    return R.PlanMasks(cfg, state, p, B, L, B * L, rows)


@pytest.mark.parametrize("name", ["tiny_shared_norm", "tiny_no_fam", "tiny_audio_only"])
def test_oracle_asks_for_every_site_in_plan_order(name):
    """The oracle's `drop` hook meets the sites in the order the plan builder numbers them (so a name can only mean one site),
    with keep-everything masks (p = 0: factor 1.0) it reproduces the plain oracle bit for bit, and real masks move the result."""
    import torch
    from oracle import m2fnet_oracle as O
    cfg, B, L, lengths, kind = synth.CASES[name]
    sd = synth.make_state_dict(cfg)
    batch = synth.make_inputs(cfg, B, L, lengths, kind)
    plain = O.loss_and_grads(sd, cfg, *batch)
    for rounding in (None, O.Bf16Rounding()):
        hook = _hook(cfg, B, L, 0.0)
        got = O.loss_and_grads(sd, cfg, *batch, rounding=rounding, drop=hook)
        assert hook.seen == list(R.site_map(cfg))
        if rounding is None:
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
            assert all(torch.equal(got[2][k], plain[2][k]) for k in plain[2])
        else:
            same = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding())
            assert torch.equal(got[0], same[0]) and all(torch.equal(got[2][k], same[2][k]) for k in same[2])
    dropped = O.loss_and_grads(sd, cfg, *batch, drop=_hook(cfg, B, L, 0.3))
    assert abs(dropped[1].item() - plain[1].item()) > 1e-3


def test_bf16_attention_emulation_with_masks_has_the_autograd_gradient():
    """_Attn16 with every rounding rule off and a mask on the probabilities is plain attention with that mask: its hand-written
    backward must equal float64 autograd."""
    import torch
    from oracle import m2fnet_oracle as O
    g = torch.Generator().manual_seed(3)
    B, L, H, hd = 2, 7, 3, 5
    q, k, v = (torch.randn(B, L, H * hd, generator=g, dtype=torch.float64) for _ in range(3))
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    key_pad[1, 4:] = True
    keep = torch.from_numpy(R.attn_mask([1, 2, 3, 4], 9, 0.4, B, H, L)).double() * R.thresh_scale(0.4)[1]
    drop = lambda name, x: x * keep
    off = O.Bf16Rounding(**{r: False for r in O.Bf16Rounding.RULES})
    dout = torch.randn(B, L, H * hd, generator=g, dtype=torch.float64)
    grads = []
    for rnd in (None, off):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        O._attn(*leaves, key_pad, H, rnd, drop=drop, name="x").backward(dout)
        grads.append([t.grad for t in leaves])
    for a, b in zip(*grads):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, a.abs().max().item())
