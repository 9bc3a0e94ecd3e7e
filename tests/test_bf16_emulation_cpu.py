"""The bf16-emulating oracle (oracle/m2fnet_oracle.py, Bf16Rounding) and the teeth of the bound tests/test_bf16_emulation_gpu.py
holds the bf16 plans to (bf16_emulation.TOL).  CPU only.

* Its custom forward / backward with every rounding rule off is the plain oracle in float64 (the hand-written backward of the
  rounded GEMMs and of the attention is the derivative autograd takes of the plain ops).
* Ablation: switching off any ONE rounding rule moves the logits or some gradient tensor by at least 3 TOL on each case the GPU
  test runs - so a kernel that stopped rounding an operand, or rounded the wrong one, fails it.  Smallest effects measured:
  bias_dy 2.2e-3 (tiny_text_only), wgrad_dy / wgrad_x / attn_o 2.3e-3 .. 4.1e-3, everything else >= 3.6e-3; 3 TOL = 3e-4.
  (tiny_odd_width, head dim 15, never rounds O, so attn_o is checked on the other two cases only.)
* Not rounding at all fails the bound on (nearly) every tensor.
"""
import pytest
import torch

import synth
import bf16_emulation as E
from oracle import m2fnet_oracle as O

CASES = ["tiny_audio_only", "tiny_text_only", "tiny_odd_width"]          # the GPU test's strict cases
ODD_WIDTH = (synth._cfg(44, 60, 60, 4, 4, 4, 1, 1, 1, a_on=False, f_on=False), 3, 7, [7, 2, 5])
_REF = {}


def _case(name):
    if name == "tiny_odd_width":
        cfg, B, L, lengths = ODD_WIDTH
        return cfg, synth.make_state_dict(cfg), synth.make_inputs(cfg, B, L, lengths, "randn")
    cfg, B, L, lengths, kind = synth.CASES[name]
    return cfg, synth.make_state_dict(cfg), synth.make_inputs(cfg, B, L, lengths, kind)


def _emulated(name):
    if name not in _REF:
        cfg, sd, batch = _case(name)
        _REF[name] = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding())
    return _REF[name]


@pytest.mark.parametrize("name", ["tiny_ragged", "tiny_odd_heads", "c2_slice"])
def test_emulation_with_every_rule_off_is_the_float64_oracle(name):
    cfg, sd, batch = _case(name)
    text, audio, kp, em = batch
    plain = O.loss_and_grads({k: v.double() for k, v in sd.items()}, cfg, text.double(), audio.double(), kp, em)
    off = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding(**{r: False for r in O.Bf16Rounding.RULES}))
    assert (plain[0] - off[0]).abs().max().item() <= 1e-12
    for k, g in plain[2].items():
        assert (g - off[2][k]).abs().max().item() <= 1e-12 * max(g.abs().max().item(), 1.0), k


@pytest.mark.parametrize("hd", [15, 16])
def test_attention_rounding_follows_the_kernel_staging_rule(hd):
    """Head dim 16 (hd % 4 == 0): slabs from the shadows, V rounded in P V and K / Q / dO / O rounded in the backward products.
    Head dim 15: fp32 slabs, only the bf16 contractions Q K^T and dO V^T round."""
    g = torch.Generator().manual_seed(hd)
    B, L, H = 2, 5, 2
    q, k, v, do = (torch.randn(B, L, H * hd, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(4))
    kp = torch.zeros(B, L, dtype=torch.bool)
    kp[1, 3:] = True
    o = O._Attn16.apply(q, k, v, kp, H, O.Bf16Rounding())
    o.backward(do.detach())
    fast = hd % 4 == 0
    heads = lambda t: t.detach().reshape(B, L, H, hd).permute(0, 2, 1, 3)
    r = lambda t, on=True: O._bf16(t) if on else t
    qh, kh, vh, doh = heads(q), heads(k), heads(v), heads(do)
    s = (r(qh) @ r(kh).transpose(-1, -2)) / hd ** 0.5
    p = torch.softmax(s.masked_fill(kp[:, None, None, :], float("-inf")), dim=-1)
    oh = p @ r(vh, fast)
    assert torch.allclose(o.detach(), oh.permute(0, 2, 1, 3).reshape(B, L, H * hd), rtol=0, atol=1e-12)
    dp = r(doh) @ r(vh).transpose(-1, -2)
    delta = (r(doh, fast) * r(oh, fast)).sum(-1, keepdim=True)
    ds = p * (dp - delta) / hd ** 0.5
    want = {"q": ds @ r(kh, fast), "k": ds.transpose(-1, -2) @ r(qh, fast), "v": p.transpose(-1, -2) @ r(doh, fast)}
    for name, t in (("q", q), ("k", k), ("v", v)):
        assert torch.allclose(heads(t.grad), want[name], rtol=0, atol=1e-12), name
    # and the two rules differ: the unrounded V of the head-dim-15 rule is not the rounded one
    assert not torch.equal(r(vh, True), vh)


@pytest.mark.parametrize("name,rule", [(n, r) for n in CASES for r in O.Bf16Rounding.RULES
                                       if not (n == "tiny_odd_width" and r == "attn_o")])   # head dim 15 reads O as fp32
def test_each_rounding_rule_moves_the_result_beyond_the_bound(name, rule):
    cfg, sd, batch = _case(name)
    ref = _emulated(name)
    lg, loss, g = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding(**{rule: False}))
    w, k = E.worst(E.errors(lg, loss, g, ref, ~batch[2]))
    assert w >= 3 * E.TOL, (rule, k, w)


@pytest.mark.parametrize("name", CASES)
def test_the_unrounded_oracle_fails_the_bound(name):
    cfg, sd, batch = _case(name)
    ref = _emulated(name)
    lg, loss, g = O.loss_and_grads(sd, cfg, *batch)
    errs = E.errors(lg, loss, g, ref, ~batch[2])
    over = sum(v > E.TOL for v in errs.values())
    assert over >= 0.9 * len(errs), (over, len(errs))


def test_bf16_rounding_is_round_to_nearest_even():
    """_bf16 rounds as m2f_bf16_bits: nearest, ties to even, on the fp32 value."""
    one = 1.0
    ulp = 2.0 ** -7                                     # bf16 spacing in [1, 2)
    x = torch.tensor([one + ulp / 2, one + 1.5 * ulp, one + ulp / 2 + 2.0 ** -20, -(one + ulp / 2)], dtype=torch.float64)
    want = torch.tensor([one, one + 2 * ulp, one + ulp, -one], dtype=torch.float64)
    assert torch.equal(O._bf16(x), want)
