"""Adversarial training on the input embeddings, the parts that need no GPU: what M2FNet.adversarial_step and train_step(input_grads=)
refuse (each by name, before an engine exists), the drop-in loop's validator and the shipped block, the C surface, and the host
replica of the perturbation's uniform start against numbers worked out by hand."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import adversarial_ref as ref  # noqa: E402
import synth  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402

BAD_NUMBERS = (-1.0, float("nan"), float("inf"), "1", True, None)
DEFAULTS = {"enabled": False, "epsilon": 1.0, "steps": 2, "step_size": None, "norm": "utterance", "modalities": None, "same_dropout": True}


def _model(**kw):
    cfg = synth._cfg(48, 64, 64, 4, 4, 4, 1, 1, 1, **kw)
    return M2FNet(cfg), synth.make_inputs(cfg, 2, 5, None, "randn", seed=1)


def test_adversarial_step_refuses_by_name_before_it_touches_a_device():
    m, (t, a, kp, y) = _model()
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="M2FNet.adversarial_step: steps must be an integer >= 1"):
            m.adversarial_step(t, a, kp, y, epsilon=1.0, steps=bad)
    for name in ("epsilon", "step_size", "init_mag"):
        for bad in BAD_NUMBERS:
            if bad is None and name != "epsilon":
                continue                                    # (step_size None = epsilon; init_mag None is covered by its type below)
            kw = {"epsilon": 1.0, name: bad}
            with pytest.raises(ValueError, match=f"M2FNet.adversarial_step: {name} must be a finite number >= 0"):
                m.adversarial_step(t, a, kp, y, **kw)
    with pytest.raises(ValueError, match="M2FNet.adversarial_step: init_mag must be a finite number >= 0"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, init_mag=None)
    for bad in ("row", "l2", None, 0):
        with pytest.raises(ValueError, match="M2FNet.adversarial_step: unknown norm"):
            m.adversarial_step(t, a, kp, y, epsilon=1.0, norm=bad)
    with pytest.raises(ValueError, match="modalities names 'video'"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, modalities=("text", "video"))
    with pytest.raises(ValueError, match="modalities is empty"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, modalities=())
    with pytest.raises(ValueError, match="M2FNet.adversarial_step: rdrop does not combine"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, rdrop=1.0)
    for name in ("normalise", "input_grads"):
        with pytest.raises(TypeError, match=f"M2FNet.adversarial_step: {name}="):
            m.adversarial_step(t, a, kp, y, epsilon=1.0, **{name: None})
    with pytest.raises(RuntimeError, match="a SAM optimizer"):
        m.adversarial_step(t, a, kp, y, types.SimpleNamespace(sam_rho=0.05), epsilon=1.0)
    DataParallelStep = type("DataParallelStep", (), {})
    with pytest.raises(RuntimeError, match="DataParallelStep"):
        m.adversarial_step(t, a, kp, y, DataParallelStep(), epsilon=1.0)
    m.set_grad_accumulation(True)
    with pytest.raises(RuntimeError, match=r"M2FNet.adversarial_step: gradient accumulation is on \(set_grad_accumulation\(True\)\)"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0)
    m.set_grad_accumulation(False)
    assert m._engine is None
    # bf16 gradients live on the engine: a stand-in that holds the buffer is enough for the refusal, which comes before any launch
    m._engine = types.SimpleNamespace(grad_bf16_buf=object(), accumulate=False)
    with pytest.raises(RuntimeError, match=r"M2FNet.adversarial_step: bf16 gradients are on \(set_grad_bf16\(True\)\)"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0)
    m._engine = None


def test_adversarial_step_refuses_a_disabled_modality_and_a_trainable_block():
    from mer_amd.crf import LinearChainCRF
    m, (t, a, kp, y) = _model(t_on=False, f_on=False)
    with pytest.raises(ValueError, match="modalities names 'text', but the text modality of this model is disabled"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, modalities=["text"])
    with pytest.raises(ValueError, match="input_grads names 'text', but the text modality of this model is disabled"):
        m.train_step(t, a, kp, y, input_grads=("text",))
    m, (t, a, kp, y) = _model()
    crf = LinearChainCRF(m.m2f_config.cls_out)
    with pytest.raises(ValueError, match="M2FNet.adversarial_step: a trainable crf= does not combine with gradient accumulation"):
        m.adversarial_step(t, a, kp, y, epsilon=1.0, steps=2, crf=crf, label_smoothing=0.0)
    assert m._engine is None


def test_train_step_input_grads_refuses_by_name():
    m, (t, a, kp, y) = _model()
    for bad in ("video", ("text", "video"), 3):
        with pytest.raises(ValueError, match="M2FNet.train_step: input_grads"):
            m.train_step(t, a, kp, y, input_grads=bad)
    with pytest.raises(ValueError, match="M2FNet.train_step: input_grads is empty"):
        m.train_step(t, a, kp, y, input_grads=())
    with pytest.raises(RuntimeError, match="M2FNet.train_step: input_grads= does not combine with optimizer="):
        m.train_step(t, a, kp, y, input_grads="text", optimizer=types.SimpleNamespace(sam_rho=None))
    with pytest.raises(ValueError, match="M2FNet.train_step: input_grads= does not combine with rdrop"):
        m.train_step(t, a, kp, y, input_grads=("text", "audio"), rdrop=1.0)
    assert m._engine is None
    m._engine = types.SimpleNamespace(grad_bf16_buf=object(), accumulate=False)
    with pytest.raises(RuntimeError, match=r"M2FNet.train_step: input_grads= does not combine with bf16 gradients \(set_grad_bf16\(True\)\)"):
        m.train_step(t, a, kp, y, input_grads="audio")
    m._engine = None
    assert runtime.input_modalities(None, True, True, "x") == 3 and runtime.input_modalities("audio", True, True, "x") == runtime.IN_AUDIO
    assert runtime.input_modalities(["text"], True, False, "x") == runtime.IN_TEXT and runtime.input_modalities(None, False, True, "x") == 2


def test_hyper_parameter_checks():
    assert runtime.check_adv_hyper(1, None, 0) == (1.0, 1.0, 0.0) and runtime.check_adv_hyper(0.5, 0.25, 2) == (0.5, 0.25, 2.0)
    assert runtime.check_adv_hyper(0.0) == (0.0, 0.0, 0.0)
    assert runtime.adv_norm_kind("utterance") == 0 and runtime.adv_norm_kind("batch") == 1
    from mer_amd import functional as MF
    x = torch.zeros(3, 8)
    for bad in BAD_NUMBERS:
        with pytest.raises(ValueError, match="adversarial_ascend: epsilon"):
            MF.adversarial_ascend(x, x.clone(), x.clone(), epsilon=bad)
    with pytest.raises(ValueError, match="adversarial_ascend: unknown norm"):
        MF.adversarial_ascend(x, x.clone(), x.clone(), norm="rows")


def test_config_block_and_settings():
    import train as tr
    import yaml
    with open(os.path.join(ROOT, "src", "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["runtime"]["adversarial"] == DEFAULTS and tr.ADVERSARIAL_DEFAULTS == DEFAULTS
    assert tr.adversarial_settings(cfg) is None and tr.adversarial_settings({}) is None and tr.adversarial_settings({"runtime": {}}) is None
    want = {k: v for k, v in DEFAULTS.items() if k != "enabled"}
    assert tr.adversarial_settings({"runtime": {"adversarial": {"enabled": True}}}) == want
    on = {"enabled": True, "epsilon": 0.5, "steps": 3, "step_size": 0.2, "norm": "batch", "modalities": ["text"], "same_dropout": False}
    assert tr.adversarial_settings({"runtime": {"adversarial": on}}) == {k: v for k, v in on.items() if k != "enabled"}
    for key, bad in (("epsilon", -1), ("epsilon", float("nan")), ("epsilon", float("inf")), ("epsilon", "1"), ("epsilon", None),
                     ("step_size", -0.5), ("step_size", True), ("steps", 0), ("steps", 1.5), ("steps", True), ("norm", "row"),
                     ("norm", None), ("modalities", []), ("modalities", "text"), ("modalities", ["video"]), ("same_dropout", 1),
                     ("enabled", 1), ("init", 0.1)):
        for enabled in (True, False):                      # (a disabled block is still checked, as the other blocks are)
            with pytest.raises(ValueError, match="runtime.adversarial"):
                tr.adversarial_settings({"runtime": {"adversarial": {"enabled": enabled, key: bad}}})
    with pytest.raises(ValueError, match="runtime.adversarial must be a mapping"):
        tr.adversarial_settings({"runtime": {"adversarial": True}})
    block = {"adversarial": {"enabled": True}}
    for other, match in (({"fused_step": False}, "fused_step: True"), ({"fused_optimizer": True}, "fused_optimizer: True"),
                         ({"grad_accumulation": 2}, "grad_accumulation > 1"), ({"grad_bf16": True}, "grad_bf16: True"),
                         ({"sam": {"enabled": True}}, "runtime.sam.enabled"), ({"rdrop": {"enabled": True}}, "runtime.rdrop.enabled")):
        with pytest.raises(ValueError, match="runtime.adversarial.enabled.*" + match):
            tr.adversarial_settings({"runtime": dict(block, **other)})
    with pytest.raises(ValueError, match="runtime.adversarial.enabled.*one process"):
        tr.adversarial_settings({"runtime": block}, world=2)
    # a disabled block refuses nothing about its neighbours
    assert tr.adversarial_settings({"runtime": {"adversarial": {"enabled": False}, "sam": {"enabled": True}, "grad_bf16": True}}) is None


def test_header_ids_signatures_and_gate():
    text = open(runtime.HEADER_PATH).read()
    assert ("M2F_BUF_ADV = 29" in text and "M2F_BUF_ADV_SKIP = 30" in text and "M2F_BUF_ADV_DELTA_TEXT = 31" in text
            and "M2F_BUF_ADV_DELTA_AUDIO = 32" in text and "M2F_BUF_LIMIT = 33" in text)
    assert (runtime.BUF_ADV, runtime.BUF_ADV_SKIP, runtime.BUF_ADV_DELTA_TEXT, runtime.BUF_ADV_DELTA_AUDIO) == (29, 30, 31, 32)
    assert f"M2F_ADV_SITE_TEXT 0x{runtime.ADV_SITE_TEXT:X}u" in text and f"M2F_ADV_SITE_AUDIO 0x{runtime.ADV_SITE_AUDIO:X}u" in text
    assert (ref.SITE_TEXT, ref.SITE_AUDIO) == (runtime.ADV_SITE_TEXT, runtime.ADV_SITE_AUDIO)
    for name in ("m2f_adv_ascend", "m2f_adv_init", "m2f_adv_scratch_bytes", "m2f_plan_adversarial", "m2f_plan_adversarial_bytes",
                 "m2f_plan_adv_begin", "m2f_plan_adv_ascend"):
        assert name in runtime.SIGNATURES and hasattr(runtime.lib(), name)
    assert runtime.lib().m2f_adv_scratch_bytes(1) == 24 and runtime.lib().m2f_adv_scratch_bytes(130) == 9 * 24
    mk = open(os.path.join(runtime.CSRC, "Makefile")).read()
    assert "adversarial.hip" in mk and "adversarial.o: GATE = check_spills.py --adv" in mk
    gated = [l for l in mk.splitlines() if l.startswith("GATED =")][0].split()
    assert "adversarial" in gated


def test_uniform_start_against_hand_computed_values():
    """State (1, 2, 3, 0).  Worked with Python integers, independently of numpy: the site key of 0xAD510001 is 0xE322BED2, the hash of
    element 0 under it 0xE8B4CCCB, so h >> 8 = 15,250,636 and 2 * 15,250,636 * 2^-24 - 1 = 0.8180174827575684; element 5 * 20 + 7 under
    0xAD510002 (key 0x0CE8E281) hashes to 0x45D2BF10: 4,575,935 -> -0.4545060396194458; element 129 * 301 + 300 under the first site
    to 0x9369B412: 9,660,852 -> 0.15166330337524414."""
    s = (1, 2, 3, 0)
    from dropout_ref import site_key
    assert int(site_key(s, ref.SITE_TEXT)) == 0xE322BED2 and int(site_key(s, ref.SITE_AUDIO)) == 0x0CE8E281
    assert int(ref.keep_hash(0xE322BED2, [0])[0]) == 0xE8B4CCCB
    u = ref.uniform_unit(s, ref.SITE_TEXT, [0, 129], 20)
    assert u.dtype == np.float32 and u.shape == (2, 20) and float(u[0, 0]) == 0.8180174827575684
    assert float(ref.uniform_unit(s, ref.SITE_AUDIO, [5], 20)[0, 7]) == -0.4545060396194458
    assert float(ref.uniform_unit(s, ref.SITE_TEXT, [129], 301)[0, 300]) == 0.15166330337524414
    # the start: one fp32 multiply by fp32(init_mag / sqrt(d))
    d0 = ref.uniform_start(s, ref.SITE_TEXT, [0], 20, 0.5)
    assert float(d0[0, 0]) == float(np.float32(0.5 / math.sqrt(20)) * np.float32(0.8180174827575684))
    big = ref.uniform_unit(s, ref.SITE_TEXT, np.arange(64), 301)
    assert big.min() >= -1.0 and big.max() < 1.0 and abs(float(big.mean())) < 0.02 and abs(float((big ** 2).mean()) - 1 / 3) < 0.02


def test_reference_ascent_properties():
    """The float64 statements themselves: the projection binds or idles as asked, zero and non-finite gradients leave delta, masked
    rows keep theirs."""
    g = torch.tensor([[3.0, 4.0], [0.0, 0.0], [float("inf"), 1.0], [1.0, 0.0]], dtype=torch.float64)
    dl = torch.tensor([[0.0, 0.0], [0.3, 0.4], [0.1, 0.0], [9.0, 9.0]], dtype=torch.float64)
    xc = torch.ones(4, 2, dtype=torch.float64)
    pad = torch.tensor([False, False, False, True])
    new, x = ref.ascend(xc, g, dl, pad, 1.0, 0.5, "utterance")
    assert torch.allclose(new[0], torch.tensor([0.3, 0.4], dtype=torch.float64)) and torch.equal(new[1], dl[1]) and torch.equal(new[2], dl[2])
    assert torch.equal(new[3], dl[3]) and torch.equal(x[3], xc[3]) and torch.equal(x[:3], xc[:3] + new[:3])
    new, _ = ref.ascend(xc[:2], g[:2], dl[:2], pad[:2], 0.25, 0.5, "utterance")
    assert torch.allclose(new.norm(dim=-1), torch.tensor([0.25, 0.25], dtype=torch.float64))
    new, _ = ref.ascend(xc[:2], g[:2], dl[:2], pad[:2], 10.0, 1.0, "batch")           # ||g|| = 5 over the batch
    assert torch.allclose(new, dl[:2] + g[:2] / 5.0)
    new, _ = ref.ascend(xc, g, dl, pad, 10.0, 1.0, "batch")                           # an inf anywhere: the batch norm is not finite
    assert torch.equal(new, dl)
