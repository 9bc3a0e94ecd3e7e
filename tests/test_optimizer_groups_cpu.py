"""Host side of parameter groups and decoupled weight decay (FusedAdam(params=...), FusedAdamW, runtime.optimizer): how src/train.py
cuts the groups from the model's (name, shape) list, the tensor -> group map the kernels walk, what the constructor refuses, and the
state_dict format - all without a GPU."""
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import synth  # noqa: E402
from mer_amd import layout, runtime  # noqa: E402
from mer_amd.model import M2FNet  # noqa: E402
from mer_amd.optim import FusedAdam, FusedAdamW  # noqa: E402

ENCODERS = ("audio_encoders", "text_encoders")


def _shipped_config():
    from utils import get_config
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        return get_config()
    finally:
        os.chdir(cwd)


def _cfg(block, lr=5e-4, wd=5e-5):
    return {"runtime": {"optimizer": block}, "solver": {"lr": lr, "weight_decay": wd}}


def _tiny():
    return M2FNet(synth.CASES["tiny_shared_norm"][0])


def _split(model):
    named = dict(model.named_parameters())
    enc = [p for n, p in named.items() if n.startswith(ENCODERS)]
    rest = [p for n, p in named.items() if not n.startswith(ENCODERS)]
    return enc, rest


# ---- 1. runtime.optimizer -> groups -----------------------------------------------------------------------------------------------
def test_shipped_config_has_the_block_and_it_means_todays_optimizer():
    import train as tr
    cfg = _shipped_config()
    block = cfg.runtime.optimizer
    assert dict(block) == {"name": "adam", "no_decay_1d": False, "lr_scale": {}, "frozen": []}
    shapes = tr.model_named_shapes(cfg.model)
    assert tr.optimizer_groups(cfg, shapes) is None
    assert tr.optimizer_groups({"solver": {"lr": 1e-3, "weight_decay": 0.0}}, shapes) is None      # no runtime block at all


def test_every_parameter_lands_in_exactly_one_group_or_in_frozen():
    import train as tr
    cfg = _shipped_config()
    shapes = tr.model_named_shapes(cfg.model)
    names = [n for n, _ in shapes]
    assert len(names) == len(set(names)) > 100
    block = {"name": "adamw", "no_decay_1d": True, "lr_scale": {"audio_encoders": 0.1, "text_encoders": 0.1}, "frozen": ["fusion_layers.0"]}
    name, groups, frozen = tr.optimizer_groups(_cfg(block), shapes)
    assert name == "adamw"
    seen = [n for g in groups for n in g["names"]] + frozen
    assert sorted(seen) == sorted(names)                       # each exactly once
    assert frozen and all(n.startswith("fusion_layers.0.") for n in frozen)
    assert not any(n.startswith("fusion_layers.0.") for g in groups for n in g["names"])
    # four groups: encoders x {decays, not}, rest x {decays, not}
    assert len(groups) == 4
    shape_of = dict(shapes)
    for g in groups:
        one_d = {len(shape_of[n]) == 1 for n in g["names"]}
        assert len(one_d) == 1                                 # no_decay_1d separates exactly the 1-D tensors
        assert g["weight_decay"] == (0.0 if one_d == {True} else 5e-5)
        enc = {n.startswith(ENCODERS) for n in g["names"]}
        assert len(enc) == 1
        assert g["lr"] == pytest.approx(5e-4 * (0.1 if enc == {True} else 1.0), rel=1e-12)
    # without no_decay_1d every tensor decays
    _, groups, _ = tr.optimizer_groups(_cfg({"name": "adamw"}), shapes)
    assert len(groups) == 1 and groups[0]["names"] == names and groups[0]["weight_decay"] == 5e-5 and groups[0]["lr"] == 5e-4
    _, groups, _ = tr.optimizer_groups(_cfg({"no_decay_1d": True}), shapes)
    assert [{len(shape_of[n]) == 1 for n in g["names"]} for g in groups] == [{False}, {True}]


def test_optimizer_block_errors_raise_before_the_gpu_is_touched():
    import train as tr
    shapes = tr.model_named_shapes(_shipped_config().model)
    for block, match in (({"name": "sgd"}, "adam or adamw"),
                         ({"no_decay_1d": 1}, "true or false"),
                         ({"lr_scale": {"audio_encoders": 0}}, "positive finite"),
                         ({"lr_scale": {"audio_encoders": True}}, "positive finite"),
                         ({"lr_scale": {"no_such_module": 0.5}}, "matches no parameter"),
                         ({"frozen": ["audio_encoder"]}, "matches no parameter"),
                         ({"lr_scale": {"audio_encoders": 0.1, "audio_encoders.0": 0.5}}, "overlap"),
                         ({"lr_scale": {"text_encoders": 0.1}, "frozen": ["text_encoders.0.layers.0"]}, "overlap"),
                         ({"frozen": ["audio_encoders", "audio_proj", "text_encoders", "text_proj", "fusion_layers", "output_layer"]},
                          "no parameter to train"),
                         ({"name": "adamw", "momentum": 0.9}, "unknown key")):
        with pytest.raises(ValueError, match=match):
            tr.optimizer_groups(_cfg(block), shapes)
    # more groups than the hyper table has rows
    many = {f"text_encoders.0.layers.{i}": 0.5 + 0.01 * i for i in range(5)}
    many.update({f"audio_encoders.0.layers.{i}": 0.3 + 0.01 * i for i in range(5)})
    with pytest.raises(ValueError, match="at most 16"):
        tr.optimizer_groups(_cfg({"no_decay_1d": True, "lr_scale": many}), shapes)
    src = inspect.getsource(tr.main)
    assert src.index("optimizer_groups(config") < src.index("init_distributed")
    assert "optimizer = build_optimizer(config, model)" in src


def test_build_optimizer_hands_the_cut_groups_to_the_fused_optimizer():
    import train as tr
    from utils import AttrDict
    model = _tiny()
    cfg = AttrDict(runtime=AttrDict(optimizer={"name": "adamw", "no_decay_1d": True, "frozen": ["audio_encoders"]}),
                   solver=AttrDict(lr=2e-3, weight_decay=0.01))
    opt = tr.build_optimizer(cfg, model)
    assert isinstance(opt, FusedAdamW) and len(opt.param_groups) == 2
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    assert all(g["decoupled_weight_decay"] and g["lr"] == 2e-3 for g in opt.param_groups)
    owned = {id(p) for g in opt.param_groups for p in g["params"]}
    for n, p in model.named_parameters():
        assert (id(p) in owned) == (not n.startswith("audio_encoders")), n
    plain = tr.build_optimizer(AttrDict(runtime=AttrDict(), solver=AttrDict(lr=2e-3, weight_decay=0.01)), model)
    assert type(plain) is FusedAdam and not plain._grouped and len(plain.param_groups) == 1


# ---- 2. the tensor -> group map, the constructor's refusals -------------------------------------------------------------------------
def test_tensor_group_map_follows_the_parameter_map():
    model = _tiny()
    enc, rest = _split(model)
    opt = FusedAdam(model, params=[{"params": rest, "lr": 1e-4}, {"params": enc[: len(enc) // 2]}])
    specs = [s for s in layout.param_specs(model.m2f_config)[0] if not s.alias_of]
    named = dict(model.named_parameters(remove_duplicate=False))
    tg = opt.tensor_group_map()
    assert len(tg) == len(specs) == len(list(model.parameters()))
    half = {id(p) for p in enc[: len(enc) // 2]}
    for s, g in zip(specs, tg):
        p = named[s.name]
        assert g == (1 if id(p) in half else -1 if s.name.startswith(ENCODERS) else 0), s.name
    assert -1 in tg and 0 in tg and 1 in tg
    # add_param_group between steps: the map follows, the new group starts at step 0
    opt.add_param_group({"params": enc[len(enc) // 2:], "weight_decay": 0.1})
    assert -1 not in opt.tensor_group_map() and opt._gsteps == [0, 0, 0]
    # today's object: one group, every tensor, not grouped; a second group makes it grouped
    plain = FusedAdam(model, lr=1e-3, weight_decay=0.01)
    assert not plain._grouped and set(plain.tensor_group_map()) == {0}
    assert FusedAdamW(model)._grouped and FusedAdam(model, params=model.parameters())._grouped
    sub = FusedAdam(model, params=rest)
    sub.add_param_group({"params": enc})
    assert sub._grouped and len(sub.param_groups) == 2


def test_constructor_refusals():
    model = _tiny()
    enc, rest = _split(model)
    with pytest.raises(ValueError, match="do not belong to the model"):
        FusedAdam(model, params=[{"params": rest}, {"params": [torch.nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError, match="do not belong to the model"):
        FusedAdamW(model, params=_tiny().parameters())
    with pytest.raises(ValueError, match="more than one parameter group"):
        FusedAdam(model, params=[{"params": enc}, {"params": rest + enc[:1]}])
    ps = list(model.parameters())
    assert len(FusedAdam(model, params=[{"params": [p]} for p in ps[:16]]).param_groups) == 16
    with pytest.raises(ValueError, match="at most 16"):
        FusedAdam(model, params=[{"params": [p]} for p in ps[:17]])
    full = FusedAdam(model, params=[{"params": [p]} for p in ps[:16]])
    with pytest.raises(ValueError, match="at most 16"):
        full.add_param_group({"params": [ps[16]]})
    for opt_name in ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused"):
        with pytest.raises(ValueError, match=opt_name):
            FusedAdam(model, **{opt_name: True})
        with pytest.raises(ValueError, match=opt_name):
            FusedAdamW(model, params=[{"params": enc, opt_name: True}, {"params": rest}])
        FusedAdam(model, **{opt_name: False})                     # torch's own default: accepted
    with pytest.raises(TypeError, match="nesterov"):
        FusedAdam(model, nesterov=True)
    with pytest.raises(ValueError, match="do not belong"):
        FusedAdam(model).add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})


def test_fused_adamw_has_torchs_defaults():
    model = _tiny()
    ours, theirs = FusedAdamW(model), torch.optim.AdamW(model.parameters())
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert ours.defaults[k] == theirs.defaults[k], k
    assert ours.defaults["weight_decay"] == 1e-2 and ours.param_groups[0]["decoupled_weight_decay"] is True
    assert FusedAdam(model, params=model.parameters()).param_groups[0]["decoupled_weight_decay"] is False
    sig = inspect.signature(FusedAdam.__init__)
    assert list(sig.parameters)[:7] == ["self", "model", "lr", "betas", "eps", "weight_decay", "max_grad_norm"]
    assert sig.parameters["params"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["decoupled_weight_decay"].default is False


# ---- 3. state_dict format -----------------------------------------------------------------------------------------------------------
def test_fresh_state_dict_has_torchs_groups_and_indices():
    model = _tiny()
    enc, rest = _split(model)

    def groups(clone):
        f = (lambda p: p.detach().clone().requires_grad_()) if clone else (lambda p: p)
        return [{"params": [f(p) for p in enc], "lr": 1e-4}, {"params": [f(p) for p in rest], "weight_decay": 0.0, "betas": (0.8, 0.99)}]
    ours = FusedAdamW(model, lr=5e-4, weight_decay=5e-4, params=groups(False)).state_dict()
    theirs = torch.optim.AdamW(groups(True), lr=5e-4, weight_decay=5e-4).state_dict()
    assert ours["state"] == {} == theirs["state"]
    assert len(ours["param_groups"]) == len(theirs["param_groups"]) == 2
    for a, b in zip(ours["param_groups"], theirs["param_groups"]):
        assert a["params"] == b["params"]                         # indices run on across the groups, as torch numbers them
        assert set(b) <= set(a), set(b) - set(a)                  # every key torch's step() reads is there
        for k in ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay"):
            assert a[k] == b[k], k
    assert ours["param_groups"][1]["params"][0] == len(enc)
    # and it loads into torch's optimizer, whose groups then still hold what its step() needs
    t = torch.optim.AdamW(groups(True), lr=1.0)
    t.load_state_dict(ours)
    assert t.param_groups[0]["lr"] == 1e-4 and t.param_groups[1]["betas"] == (0.8, 0.99) and t.param_groups[0]["amsgrad"] is False


# ---- 4. the C entries -----------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_gated():
    header = open(os.path.join(ROOT, "include", "m2fnet_hip.h")).read()
    for sym in ("m2f_adam_hyper_groups", "m2f_adam_step_grouped", "m2f_plan_fused_adam_setup_grouped"):
        assert sym in runtime.SIGNATURES and f"int {sym}(" in header, sym
    assert "#define M2F_ADAM_MAX_GROUPS 16" in header and runtime.ADAM_MAX_GROUPS == 16
    import ctypes
    assert ctypes.sizeof(runtime.AdamGroupC) == 32              # double, 4 floats, 2 ints: m2f_adam_group
    mk = open(os.path.join(ROOT, "multimodal-emotion-recognition_amd", "csrc", "Makefile")).read()
    assert "check_spills.py --adam" in mk
