"""Train-mode plans with dropout ON against the float64 oracle run under the device's own masks.

A train plan draws its masks from (engine.rng, site, element index); tests/golden/dropout_ref.py reproduces that function on the
host, names the sites in the order csrc/plan_build.hip numbers them and lays the masks out as the oracle sees the batch, and
oracle/m2fnet_oracle.py applies them through its `drop` hook where the reference applies its dropouts.  So the dropout-on forward,
loss and EVERY parameter gradient meet an independent reference: a site indexed by the leading dimension, packed and padded plans
indexing differently, a wrong 1 / (1 - p) at one site, two sites sharing a key, a dropout on the wrong side of a residual, the
attention index built from the batch's L on a bucketed plan, a graph replay that advances the counter by the wrong amount - each
moves logits, loss or a gradient far beyond these bounds.

The rng state is READ BACK from the device, never recomputed.  forward / loss / backward run without advancing it, as
test_model_gpu.py::test_dropout_backward_consistent_with_forward_mask does.
Bounds, fp32 mode: the dropout = 0 bounds of test_model_gpu.py - loss 2e-5, gradients 3e-5 + 1e-3 max|ref|, logits 1e-4.
bf16 mode: tests/golden/bf16_emulation.TOL against the Bf16Rounding oracle with the same masks (see the bf16 tests below).
Every case prints its errors before it asserts.

Measured on MI355X (fp32 mode, every case met the project's bounds as they stand, so none rests on a measured error):
  case                 logits    loss      worst gradient / its bound
  tiny_ragged 0.3      2.0e-7    2.2e-8    2.1e-4 (output_layer.3.weight)        padded 8 x 16
  tiny_shared_norm     9.7e-8    7.7e-8    2.8e-4 (output_layer.7.weight)        padded 4 x 16
  tiny_odd_heads       1.1e-7    1.2e-7    2.7e-4 (output_layer.5.bias)          padded 4 x 48
  tiny_no_fam          2.2e-7    1.0e-7    2.8e-4 (audio out_proj.bias)          padded 4 x 16
  tiny_audio_only      2.3e-7    2.7e-7    4.4e-4 (audio in_proj_bias)           padded 4 x 16
  tiny_ragged 0.5      3.1e-7    2.0e-7    3.6e-4 (audio_proj.weight)            padded 8 x 16
  packed_tiny          1.8e-7    8.9e-8    2.1e-4 (output_layer.3.weight)        packed, T = 64
  long_tiny            2.6e-7    4.5e-8    2.5e-4 (output_layer.3.bias)          packed 4 x 128, T = 320
  input gradients      2.0e-7    2.2e-8    2.1e-4 (74 tensors, text and audio gradients among them)
  graph replay         |loss - oracle| <= 2e-7 at step counters 1, 2, 3
The float64 oracle's own fp32 run is 1e-7 (logits) and 2e-7 (loss) away from it under the same masks.
"""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import synth  # noqa: E402
import long_cases  # noqa: E402
import bf16_emulation as E  # noqa: E402
import dropout_ref as R  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from oracle import m2fnet_oracle as O  # noqa: E402

TOL_LOSS, TOL_LOGITS = 2e-5, 1e-4


def _grad_bound(ref):
    return 3e-5 + 1e-3 * ref.abs().max().item()


# name -> (cfg, B, L, lengths, packed)
def _case(name):
    if name in synth.CASES:
        cfg, B, L, lengths, _ = synth.CASES[name]
        return cfg, B, L, lengths, False
    if name == "packed_tiny":                      # tests/test_packed_gpu.py::_ragged_case("tiny"): 46 valid rows of 8 x 16 slots
        return synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1), 6, 16, [16, 3, 9, 1, 12, 5], True
    cfg, B, L, lengths = long_cases.CASES[name]    # L > 64: always a packed plan on the long-dialogue kernels
    return cfg, B, L, lengths, True


def _double_sd(sd):
    seen = {}
    return {k: seen.setdefault(id(v), v.double()) for k, v in sd.items()}


def _model(cfg, sd, precision, packed):
    torch.manual_seed(20261017)                    # the engine seeds its rng from torch's seed: the same masks in every run
    m = M2FNet(cfg, precision=precision, packed=packed)
    m.load_state_dict(sd)
    return m.to("cuda").train()


def _plan_grads(m):
    eng = m.engine()
    by_id = {id(p): k for k, p in m.named_parameters()}
    return {by_id[id(p)]: eng.flat_grad[o: o + n].view(s).detach().cpu() for (p, o, n, s) in eng.items}


def _run_plan(name, p_drop, precision="fp32", outputs=(0, True)):
    """One forward / loss / backward of a train plan with dropout on, the rng state as read from the device, and the oracle's
    hook for exactly those masks."""
    cfg, B, L, lengths, packed = _case(name)
    cfg = dict(cfg, dropout=p_drop)
    sd = synth.make_state_dict(cfg)
    batch = synth.make_inputs(cfg, B, L, lengths, "randn")
    m = _model(cfg, sd, precision, packed)
    eng = m.engine()
    valid = int((~batch[2]).sum()) if packed else None
    plan = eng.plan(B, L, True, True, valid, outputs)
    assert plan.packed == packed and plan.train and plan.cfg.dropout > 0
    plan.set_inputs(*[t.cuda() for t in batch])
    state = R.state_of(eng.rng)
    plan.forward()
    loss = plan.loss_fwd(0.1, False, True)[0].item()
    plan.backward()
    torch.cuda.synchronize()
    assert R.state_of(eng.rng) == state, "forward / loss / backward must not advance the rng"
    masks = R.PlanMasks.of_plan(cfg, plan, state, B, L)
    return cfg, sd, batch, m, plan, loss, masks


def _compare_fp32(label, cfg, sd, batch, m, plan, loss, masks, input_grads=False):
    text, audio, key_pad, emotion = batch
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(_double_sd(sd), cfg, text.double(), audio.double(), key_pad, emotion, drop=masks,
                                                       input_grads=input_grads)
    assert masks.seen == list(R.site_map(cfg)), "the oracle must have met every site of the plan, in the plan's order"
    valid = ~key_pad
    e_logits = (plan.logits.cpu().double() - ref_logits)[valid].abs().max().item()
    e_loss = abs(loss - ref_loss.item())
    grads = _plan_grads(m)
    if input_grads:
        grads["text"] = plan.input_grad(runtime.IN_TEXT).cpu() * valid[..., None]
        grads["audio"] = plan.input_grad(runtime.IN_AUDIO).cpu() * valid[..., None]
        ref_grads = dict(ref_grads, text=ref_grads["text"] * valid[..., None], audio=ref_grads["audio"] * valid[..., None])
    worst = (0.0, "")
    bad = []
    for k, g in grads.items():
        ref = ref_grads[k]
        err = (g.double() - ref).abs().max().item()
        worst = max(worst, (err / _grad_bound(ref), k))
        if err > _grad_bound(ref):
            bad.append((k, err, _grad_bound(ref)))
    print(f"{label}: logits err {e_logits:.2e} (bound {TOL_LOGITS}), loss err {e_loss:.2e} (bound {TOL_LOSS}), worst gradient at "
          f"{worst[0]:.2e} of its bound ({worst[1]}) over {len(grads)} tensors; plan {plan.B} x {plan.L}, T = {plan.T}, packed {plan.packed}")
    assert e_logits < TOL_LOGITS, (label, e_logits)
    assert e_loss < TOL_LOSS, (label, loss, ref_loss.item())
    assert not bad, (label, bad[:5])
    assert len(grads) >= 10


@pytest.mark.parametrize("name,p_drop", [("tiny_ragged", 0.3), ("tiny_shared_norm", 0.3), ("tiny_odd_heads", 0.3), ("tiny_no_fam", 0.3),
                                         ("tiny_audio_only", 0.3), ("tiny_ragged", 0.5), ("packed_tiny", 0.3), ("long_tiny", 0.3)])
def test_dropout_on_plan_matches_float64_oracle_under_its_own_masks(name, p_drop):
    """Padded plans on shape buckets (tiny_ragged: 5 x 9 -> 8 x 16, so the plan's L is not the batch's), a packed plan (rows
    cu[b] + i), and a long-dialogue plan (L = 110 -> 128, attention_dlong.hip)."""
    cfg, sd, batch, m, plan, loss, masks = _run_plan(name, p_drop)
    if name == "tiny_ragged":
        assert (plan.B, plan.L) == (8, 16)
    if name in ("packed_tiny", "long_tiny"):
        assert plan.packed and plan.T < plan.B * plan.L
    _compare_fp32(f"{name} p={p_drop}", cfg, sd, batch, m, plan, loss, masks)


def test_dropout_on_input_gradients_match_float64_oracle():
    """m2f_plan_backward_outputs(text | audio): d loss / d text and d loss / d audio pass the pre-projection dropout (the NN GEMM
    with a site) and every encoder-layer site on their way back."""
    cfg, sd, batch, m, plan, loss, masks = _run_plan("tiny_ragged", 0.3, outputs=(runtime.IN_TEXT | runtime.IN_AUDIO, True))
    assert plan.input_mask == 3
    _compare_fp32("tiny_ragged input gradients", cfg, sd, batch, m, plan, loss, masks, input_grads=True)


def _per_dialogue(logits, ref_logits, key_pad):
    scale = ref_logits[~key_pad].abs().max().item()
    d = (logits.double() - ref_logits.double()).abs().amax(-1)
    d[key_pad] = 0
    return (d.amax(1) / scale).tolist()


def _emulate_fp32(sd, cfg, batch, masks):
    """The Bf16Rounding oracle with the same masks in fp32 arithmetic instead of float64 -> (logits, loss, grads).  Not called by
    the tests: the recipe by which tests/golden/dropout_bf16_own_distance_c2_slice.json was measured (bf16_emulation.errors of
    this against the float64 run of O.loss_and_grads, the masks of the rng state the file names)."""
    text, audio, key_pad, emotion = batch
    leaves = {}
    sd2 = {k: leaves.setdefault(id(v), v.detach().clone().requires_grad_(True)) for k, v in sd.items()}
    logits = O.forward(sd2, cfg, text, audio, key_pad, rnd=O.Bf16Rounding(), drop=masks)
    loss = O.cross_entropy(logits, emotion)
    loss.backward()
    return logits.detach(), loss.detach(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in sd2.items()}


# bf16 cases -> None: held to bf16_emulation.TOL itself; or the file under tests/golden that records the emulation's own
# fp32-against-float64 distance PER TENSOR (relative, as bf16_emulation.errors measures: logits, loss, every gradient).
#   tiny_ragged  MI355X: worst tensor 8.5e-6 (text_encoders.0.layers.1.linear2.weight), logits 4.3e-8, every dialogue below 5e-8 -
#                inside TOL = 1e-4 with these masks (without dropout the case is in test_bf16_emulation_gpu.py's FLIPPED list).
#                The emulation's own distance is 3.3e-3 (in_proj_weight of text layer 1): it flips where the plan does not.
#   c2_slice     cannot meet TOL with no kernel at fault, as test_bf16_emulation_gpu.py documents for this case without dropout
#                ("not compared"): at width 768 some value always sits within fp32 noise of a bf16 rounding midpoint, rounds the
#                other way under another summation order, and the one-ulp change spreads through its dialogue and the weight
#                gradients.  So the reference is measured against itself - the same emulation, the same masks, fp32 arithmetic
#                instead of float64 (`_emulate_fp32`), on the CPU with 16 and with 4 threads, the larger of the two per tensor -
#                and EACH tensor is bounded by four times ITS OWN distance (or TOL): logits 3.316e-3, loss 4.531e-5, gradients
#                from 1.05e-3 (output_layer.3.bias) to 3.449e-1 (output_layer.0.weight; one flip that fp32 arithmetic takes the
#                same way on CPU and GPU).  Observed on MI355X: logits 3.83e-3, loss 2.7e-5, worst gradient tensor 3.449e-1
#                (output_layer.0.weight), per-dialogue logit errors 3.8e-3 1.4e-3 6.2e-4 1.7e-3; the worst ratio of a tensor's
#                error to its bound is printed by every run (PER_TENSOR_RATIO below).  The counter-check at the end shows
#                that the emulation under the NEXT step's masks is far outside the logits / loss bounds.
BF16_OWN_DISTANCE = {"tiny_ragged": None, "c2_slice": "dropout_bf16_own_distance_c2_slice.json"}


@pytest.mark.parametrize("name", sorted(BF16_OWN_DISTANCE))
def test_dropout_on_bf16_plan_matches_rounding_oracle_under_its_own_masks(name, golden_dir):
    """bf16 mode against the Bf16Rounding oracle (float64, rounding where the kernels round, the masks applied to the fp32
    epilogue values in front of the next operand rounding) with the plan's own masks; compared as
    tests/test_bf16_emulation_gpu.py compares: max |plan - emulation| / max |emulation| per tensor - logits (valid rows), loss,
    every gradient - against bf16_emulation.TOL, or where that cannot be met four times the emulation's own fp32 / float64
    distance of the same tensor (BF16_OWN_DISTANCE)."""
    cfg, sd, batch, m, plan, loss, masks = _run_plan(name, 0.3, precision="bf16")
    ref = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding(), drop=masks)
    assert masks.seen == list(R.site_map(cfg))
    valid = ~batch[2]
    errs = E.errors(plan.logits.cpu(), loss, _plan_grads(m), ref, valid)
    w, k = E.worst(errs)
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    per = _per_dialogue(plan.logits.cpu(), ref[0], batch[2])
    print(f"{name} bf16 p=0.3: worst {w:.3e} ({k}) over {len(errs)} tensors, logits {errs['logits']:.2e}, loss {errs['loss']:.2e}; next "
          f"{', '.join(f'{n} {v:.2e}' for n, v in top[1:])}; per-dialogue logit error {', '.join(f'{x:.1e}' for x in per)}")
    assert len(errs) >= 10
    own = BF16_OWN_DISTANCE[name]
    if own is None:
        assert w <= E.TOL, (name, k, w, top)
        return
    with open(os.path.join(golden_dir, own)) as f:
        rec = json.load(f)
    assert rec["rng_state"] == masks.state, "the recorded distances belong to other masks"
    assert set(rec["distance"]) == set(errs), set(rec["distance"]) ^ set(errs)
    bound = {n: max(4 * rec["distance"][n], E.TOL) for n in errs}
    ratio = {n: errs[n] / bound[n] for n in errs}
    rk = max(ratio, key=ratio.get)
    print(f"{name}: PER_TENSOR_RATIO error / max(4 x own distance, TOL): worst {ratio[rk]:.3f} ({rk}: {errs[rk]:.2e} of {bound[rk]:.2e}); "
          f"logits {ratio['logits']:.3f}, loss {ratio['loss']:.3f}")
    bad = {n: (errs[n], bound[n]) for n in errs if errs[n] > bound[n]}
    assert not bad, (name, bad)
    # the masks matter at this bound: the emulation under the next step's masks is far outside it
    state = list(masks.state)
    state[2] += 1
    other = O.loss_and_grads(sd, cfg, *batch, rounding=O.Bf16Rounding(), drop=R.PlanMasks.of_plan(cfg, plan, state, *batch[2].shape))
    off = E.errors(plan.logits.cpu(), loss, {}, other, valid)
    print(f"{name}: against the emulation under the next step's masks: logits {off['logits']:.2e}, loss {off['loss']:.2e}")
    assert off["logits"] > 4 * bound["logits"] and off["loss"] > 4 * bound["loss"], off


def test_graph_replay_draws_the_masks_of_each_step_counter():
    """Three train_step(use_graph=True) calls on fixed parameters (warm-up, capture, replay): the loss of call k is the oracle's
    loss under the masks of the step counter read back after the call, the counter moves by one per call, the losses differ."""
    cfg, B, L, lengths, _ = _case("tiny_ragged")
    cfg = dict(cfg, dropout=0.3)
    sd = synth.make_state_dict(cfg)
    batch = synth.make_inputs(cfg, B, L, lengths, "randn")
    m = _model(cfg, sd, "fp32", False)
    dev = [t.cuda() for t in batch]
    sd64 = _double_sd(sd)
    losses, steps = [], []
    start = R.state_of(m.engine().rng)
    for call in range(3):
        loss = m.train_step(*dev, use_graph=True).item()
        torch.cuda.synchronize()
        eng = m.engine()
        state = R.state_of(eng.rng)
        plan = next(iter(eng.plans.values()))
        masks = R.PlanMasks.of_plan(cfg, plan, state, B, L)
        _, ref_loss, _ = O.loss_and_grads(sd64, cfg, batch[0].double(), batch[1].double(), batch[2], batch[3], drop=masks)
        print(f"call {call}: rng {state}, loss {loss:.7f}, oracle {ref_loss.item():.7f}")
        assert abs(loss - ref_loss.item()) < TOL_LOSS, (call, loss, ref_loss.item())
        losses.append(loss)
        steps.append(state[2])
        assert state[:2] == start[:2] and state[3] == start[3]
    assert steps == [start[2] + 1, start[2] + 2, start[2] + 3], (start, steps)
    assert len(set(losses)) == 3


def test_no_encoder_stack_with_dropout_refuses_a_train_plan_and_evaluates():
    """n_transformers = 0 with dropout > 0: the pre-projection dropout has no launch to ride on, the builder refuses the train
    plan with its message; the eval plan of that config matches the oracle."""
    cfg = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1, nt_a=0, dropout=0.3)
    sd = synth.make_state_dict(cfg)
    B, L, lengths = 3, 7, [7, 2, 5]
    text, audio, key_pad, emotion = synth.make_inputs(cfg, B, L, lengths, "randn")
    m = _model(cfg, sd, "fp32", False)
    dev = [t.cuda() for t in (text, audio, key_pad, emotion)]
    with pytest.raises(runtime.HipError, match="n_transformers = 0 with dropout > 0 runs in eval mode only"):
        m.train_step(*dev, use_graph=False)
    m.eval()
    with torch.no_grad():
        logits = m(*dev[:3]).cpu()
    ref = O.forward(sd, cfg, text, audio, key_pad)
    err = (logits - ref)[~key_pad].abs().max().item()
    print(f"eval plan of the refused config: logits err {err:.2e}")
    assert err < TOL_LOGITS
