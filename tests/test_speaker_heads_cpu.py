"""Host side of speaker-aware attention heads (M2FNet(speaker_heads=(n_same, n_other))): the restatement the GPU tests take their
reference values from (tests/golden/speaker_heads_ref.py) against torch's own boolean attn_mask= / src_mask= arguments on the rows
that see a key, exact zeros on the rows that see none, the head-class rule, the refused settings and ids, the plan keys, src/dataset.py's
speaker ids and collate, the config check of src/train.py, and the snapshot's `speakers` field through select / cpu / to / state_dict."""
import ctypes
import os
import sys

import pandas as pd
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "src"))

import band_ref as BR  # noqa: E402
import position_bias_ref as PB  # noqa: E402
import speaker_heads_ref as R  # noqa: E402
import synth  # noqa: E402
from mer_amd import runtime, streaming  # noqa: E402
from mer_amd.model import FusionAttentionModule, M2FNet, _Engine  # noqa: E402
from mer_amd.streaming import StreamSnapshot  # noqa: E402

TOL = 1e-12
H = 4
HEADS = (1, 1)
BANDS = [(None, None), (None, 0), (2, 0)]
PATTERNS = {"issue": lambda b, i: (3 * i + b) % 3,              # (3 i + b) % 3 = b % 3: every dialogue a monologue
            "turns": lambda b, i: ((i // 2) + b) % 3}           # three speakers in turns of two


def _case(B, L, E, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    audio = torch.randn(B, L, E, generator=g, dtype=torch.float64)
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    return text, audio, key_pad


def _speakers(B, L, pattern):
    f = PATTERNS[pattern]
    return torch.tensor([[f(b, i) for i in range(L)] for b in range(B)], dtype=torch.int64)


def _bool_mask(key_pad, band, spk):
    """the boolean attn_mask torch's modules take, [B*H, L, L] (True = not allowed), and the rows of it that see a key"""
    B, L = key_pad.shape
    hid = BR.band_mask(L, *band)[None, None].expand(B, H, L, L) | R.speaker_hidden(spk, H, HEADS)
    sees = ~(hid | key_pad[:, None, None, :]).all(-1)                     # [B, H, L]
    # a row torch would turn into NaN (it sees no key) is opened up for torch alone: those rows are compared with exact zeros instead
    open_rows = ~sees
    hid = hid & ~open_rows[..., None]
    return hid.reshape(B * H, L, L), sees


def _check_rows(sees, key_pad):
    """the compared rows are at least half of all (b, h, i) rows of valid queries - the reference alone decides this"""
    valid = (~key_pad)[:, None, :].expand_as(sees)
    frac = (sees & valid).sum().item() / valid.sum().item()
    print(f"rows that see a key: {frac:.3f} of the valid queries' rows")
    assert frac >= 0.5, frac
    return valid


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("band", BANDS, ids=str)
def test_fusion_form_agrees_with_torch_multihead_attention(band, pattern):
    """query = text, key = audio, value = text (the fusion module's call) with a boolean attn_mask [B*H, L, L]"""
    B, L, E = 3, 9, 32
    text, audio, key_pad = _case(B, L, E, [9, 4, 1], seed=1)
    spk = _speakers(B, L, pattern)
    mha = torch.nn.MultiheadAttention(E, H, batch_first=True, dtype=torch.float64).eval()
    mask, sees = _bool_mask(key_pad, band, spk)
    valid = _check_rows(sees, key_pad)
    with torch.no_grad():
        want, _ = mha(text, audio, text, key_padding_mask=key_pad, attn_mask=mask, need_weights=False)
        w, b = mha.in_proj_weight, mha.in_proj_bias
        q, k, v = text @ w[:E].T + b[:E], audio @ w[E:2 * E].T + b[E:2 * E], text @ w[2 * E:].T + b[2 * E:]
        o, p = R.attention(q, k, v, key_pad, H, return_probs=True, band=band, speakers=spk, heads=HEADS)
        # per head: torch's output before the out-projection is not exposed, so compare the heads one at a time through it
        hd = E // H
        _, pw = mha(text, audio, text, key_padding_mask=key_pad, attn_mask=mask, need_weights=True, average_attn_weights=False)
    rows = sees & valid                                                   # [B, H, L]
    assert (p - pw).abs()[rows].max().item() <= TOL
    empty = ~sees
    assert torch.all(p[empty] == 0), "a row that sees no key: P exactly 0"
    oh = o.reshape(B, L, H, hd).permute(0, 2, 1, 3)
    assert torch.all(oh[empty] == 0), "... and a zero output slice of that head"
    # the whole module on the queries all of whose heads see a key
    full = (sees | ~valid).all(1) & ~key_pad                              # [B, L]
    got = o @ mha.out_proj.weight.T + mha.out_proj.bias
    if full.any():
        assert (got - want).abs()[full].max().item() <= TOL
    hidden = R.speaker_hidden(spk, H, HEADS)
    assert hidden.any() and torch.all(p[hidden] == 0)


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_self_attention_agrees_with_a_transformer_encoder_layer(pattern):
    """one nn.TransformerEncoderLayer (post-norm, ReLU, no dropout) with src_mask = the boolean mask, on the queries all of whose
    heads see a key; the oracle's layer arithmetic restated around speaker_heads_ref.attention"""
    B, L, E = 3, 9, 32
    band = (None, None) if pattern == "turns" else (None, 0)
    text, _, key_pad = _case(B, L, E, [9, 4, 1], seed=2)
    spk = _speakers(B, L, pattern)
    if pattern == "issue":
        heads = (1, 0)                                                    # (monologues: an other-speaker head would empty every row)
    else:
        heads = HEADS
    layer = torch.nn.TransformerEncoderLayer(E, H, dim_feedforward=48, dropout=0.0, batch_first=True, dtype=torch.float64).eval()
    hid = BR.band_mask(L, *band)[None, None].expand(B, H, L, L) | R.speaker_hidden(spk, H, heads)
    sees = ~(hid | key_pad[:, None, None, :]).all(-1)
    hid = hid & sees[..., None]
    mask = hid.reshape(B * H, L, L)
    with torch.no_grad():
        # (the fused fast path of the layer takes no per-head mask on every version: the plain path is forced by a hook-free call in train-free
        # mode with a mask that requires it)
        want = layer(text, src_mask=mask, src_key_padding_mask=key_pad)
        sa = layer.self_attn
        w, b = sa.in_proj_weight, sa.in_proj_bias
        q, k, v = text @ w[:E].T + b[:E], text @ w[E:2 * E].T + b[E:2 * E], text @ w[2 * E:].T + b[2 * E:]
        att = R.attention(q, k, v, key_pad, H, band=band, speakers=spk, heads=heads)
        x = layer.norm1(text + (att @ sa.out_proj.weight.T + sa.out_proj.bias))
        got = layer.norm2(x + layer.linear2(torch.relu(layer.linear1(x))))
    full = sees.all(1) & ~key_pad
    assert full.sum().item() * 2 >= (~key_pad).sum().item()
    assert (got - want).abs()[full].max().item() <= TOL


# ---- the rule, the settings, the ids -----------------------------------------------------------------------------------------------------
def test_head_class_rule():
    for heads_n in (3, 4, 5, 8):
        for a in range(heads_n + 1):
            for b in range(heads_n + 1 - a):
                got = [runtime.speaker_head_class(h, a, b) for h in range(heads_n)]
                want = [runtime.SPK_SAME] * a + [runtime.SPK_OTHER] * b + [runtime.SPK_NONE] * (heads_n - a - b)
                assert got == want == [R.head_class(h, (a, b)) for h in range(heads_n)]
    assert (runtime.SPK_NONE, runtime.SPK_SAME, runtime.SPK_OTHER) == (R.NONE, R.SAME, R.OTHER) == (0, 1, 2)


def test_refused_settings_and_ids():
    assert runtime.speaker_heads(None) is None
    assert runtime.speaker_heads((1, 1)) == (1, 1) and runtime.speaker_heads([2, 0], {"x": 2}) == (2, 0)
    with pytest.raises(ValueError, match="at least one"):
        runtime.speaker_heads((0, 0))
    for bad in ((-1, 1), (1.0, 1), (True, 1), "11", (1,), 3):
        with pytest.raises(ValueError, match="speaker heads"):
            runtime.speaker_heads(bad)
    with pytest.raises(ValueError, match="exceeds the 4 heads of the text encoder"):
        runtime.speaker_heads((3, 2), {"the audio encoder": 8, "the text encoder": 4})
    ok = torch.tensor([[0, 255, 7]])
    for dt in (torch.uint8, torch.int32, torch.int64):
        got = runtime.speaker_ids(ok.to(dt))
        assert got.dtype == torch.uint8 and torch.equal(got.long(), ok)
    for bad in (256, -1):
        with pytest.raises(ValueError, match="0 .. 255"):
            runtime.speaker_ids(torch.tensor([[0, bad]]))
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.int16), [0, 1], None):
        with pytest.raises(ValueError, match="uint8 / int32 / int64"):
            runtime.speaker_ids(bad)


def test_model_setting_without_a_device():
    cfg = synth.CASES["tiny_ragged"][0]                                   # 4 heads at every site
    assert M2FNet(cfg).speaker_heads is None and M2FNet(cfg, speaker_heads=None).speaker_heads is None
    m = M2FNet(cfg, speaker_heads=(1, 1), context=(None, 0), position_bias=1.0)
    assert m.speaker_heads == (1, 1) and m.context == (None, 0) and m.position_bias == 1.0
    m.set_speaker_heads(2, 2)
    assert m.speaker_heads == (2, 2)
    m.set_speaker_heads(3)
    assert m.speaker_heads == (3, 0)
    for bad in ((3, 2), (0, 0), (-1, 1)):
        with pytest.raises(ValueError):
            m.set_speaker_heads(*bad)
        with pytest.raises(ValueError):
            M2FNet(cfg, speaker_heads=bad)
    assert m.speaker_heads == (3, 0)                                      # (a refused setting changes nothing)
    with pytest.raises(ValueError, match=r"exceeds the \d heads of the"):
        m.set_speaker_heads(4, 1)
    odd = synth.CASES["tiny_odd_heads"][0]                                # 4, 3 and 2 heads
    assert M2FNet(odd, speaker_heads=(1, 1)).speaker_heads == (1, 1)
    with pytest.raises(ValueError, match="exceeds the 2 heads of"):
        M2FNet(odd, speaker_heads=(2, 1))
    m.set_speaker_heads(None)
    assert m.speaker_heads is None
    assert set(M2FNet(cfg, speaker_heads=(1, 1)).state_dict()) == set(M2FNet(cfg).state_dict())       # (no parameters)
    # `speakers` on a model without the setting, and the reverse: refused before the device is looked for
    t, a, kp = torch.zeros(2, 3, 64), torch.zeros(2, 3, 48), torch.zeros(2, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match="no speaker heads"):
        M2FNet(cfg)(t, a, kp, speakers=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pass speakers="):
        M2FNet(cfg, speaker_heads=(1, 1))(t, a, kp)
    with pytest.raises(ValueError, match="0 .. 255"):
        M2FNet(cfg, speaker_heads=(1, 1))(t, a, kp, speakers=torch.full((2, 3), 256))
    assert FusionAttentionModule(16, 4, 0.0).speaker_heads is None
    assert FusionAttentionModule(16, 4, 0.0, speaker_heads=(1, 2)).speaker_heads == (1, 2)
    with pytest.raises(ValueError, match="exceeds"):
        FusionAttentionModule(16, 4, 0.0, speaker_heads=(4, 1))


def test_default_plan_key_is_what_it_was_and_a_setting_has_its_own():
    old = (8, 16, None, True, False, runtime.F32)
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32) == old
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), None, None) == old
    biased = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0), 1.0)
    assert _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0), 1.0, None) == biased
    a = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), None, (1, 1))
    b = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, None), None, (2, 0))
    c = _Engine.plan_key(8, 16, None, True, False, runtime.F32, (0, True), (None, 0), 1.0, (1, 1))
    assert a[:6] == old and c[:len(biased)] == biased and a[-1] == ("speaker_heads", 1, 1)
    assert len({old, biased, a, b, c}) == 5


def test_new_entries_are_declared():
    """The plan-level entries, the advance launches, and the kernel-level entries that CARRY the speaker heads, as the n_same / n_other
    / ids fields of their options descriptor.  The per-feature entries (base name + "_speakers") are gone from the header, the bindings
    and the library."""
    header = open(runtime.HEADER_PATH).read()
    carriers = {"m2f_attention_fwd": ("m2f_attn_opts", ("speakers",)), "m2f_attention_varlen_fwd": ("m2f_attn_opts", ("speakers",)),
                "m2f_attention_stream": ("m2f_attn_stream_opts", ("spk_cache", "spk_new")),
                "m2f_attention_stream_chunk": ("m2f_attn_stream_opts", ("spk_cache", "spk_new"))}
    mirror = {"m2f_attn_opts": runtime.AttnOptsC, "m2f_attn_stream_opts": runtime.AttnStreamOptsC}
    for sym in tuple(carriers) + ("m2f_plan_attention_speakers", "m2f_plan_get_attention_speakers", "m2f_plan_stream_speakers",
                                  "m2f_stream_advance_speakers", "m2f_stream_advance_speakers_n", "m2f_attention_speaker_class"):
        assert sym in runtime.SIGNATURES and ("int " + sym + "(") in header, sym
    for sym, (name, ids) in carriers.items():
        struct = header[header.index("typedef struct " + name + " {"):header.index("} " + name + ";")]
        fields = dict(mirror[name]._fields_)
        assert "int n_same, n_other;" in struct and fields["n_same"] is ctypes.c_int and fields["n_other"] is ctypes.c_int, name
        for f in ids:
            assert ("const uint8_t* " + f + ";") in struct and fields[f] is ctypes.c_void_p, (name, f)
        assert runtime.SIGNATURES[sym][1][-1] is ctypes.POINTER(mirror[name]), sym
        old = sym + "_speakers"
        assert old not in runtime.SIGNATURES and old not in header and not hasattr(runtime.lib(), old), old
    assert "M2F_BUF_SPEAKERS = 19" in header and runtime.BUF_SPEAKERS == 19 and runtime.BUF_STREAM_SPEAKERS == 20


# ---- the drop-in loop's host side ----------------------------------------------------------------------------------------------------
def test_dataset_speaker_ids_on_a_three_row_table():
    import dataset as ds
    table = pd.DataFrame({"Utterance": ["c", "a", "b"], "Emotion": ["joy", "anger", "neutral"], "Dialogue_ID": [0, 0, 0],
                          "Utterance_ID": [2, 0, 1], "Speaker": ["Ross", "Rachel", "Ross"]})
    emb = torch.arange(6, dtype=torch.float32).view(3, 2)
    d = ds.Dataset("train", text_embeddings=emb, audio_embeddings=emb, table=table.copy(), speakers=True)
    item = d[0]                                                           # utterance order: Rachel, Ross, Ross
    assert item["speaker"].tolist() == [0, 1, 1] and item["speaker"].dtype == torch.int64
    assert "speaker" not in ds.Dataset("train", text_embeddings=emb, audio_embeddings=emb, table=table.copy())[0]
    two = pd.concat([table, pd.DataFrame({"Utterance": ["x"], "Emotion": ["joy"], "Dialogue_ID": [1], "Utterance_ID": [0], "Speaker": ["Ross"]})],
                    ignore_index=True)
    emb4 = torch.arange(8, dtype=torch.float32).view(4, 2)
    d2 = ds.Dataset("train", text_embeddings=emb4, audio_embeddings=emb4, table=two, speakers=True)
    batch = ds.collate_fn([d2[0], d2[1]])
    assert batch["speaker"].tolist() == [[0, 1, 1], [0, 0, 0]] and batch["speaker"].dtype == torch.int64      # (ids are per dialogue; pads: 0)
    assert batch["padding_mask"].tolist() == [[False] * 3, [False, True, True]]
    assert "speaker" not in ds.collate_fn([ds.Dataset("train", text_embeddings=emb, audio_embeddings=emb, table=table.copy())[0]])
    with pytest.raises(ValueError, match="Speaker column"):
        ds.Dataset("train", text_embeddings=emb, audio_embeddings=emb, table=table.drop(columns=["Speaker"]), speakers=True)
    assert ds.dialogue_speaker_ids(["b", "a", "b", "z"], [[1, 0, 2], [3]]).tolist() == [1, 0, 1, 0]


def test_config_check_of_the_loop(monkeypatch):
    monkeypatch.chdir(ROOT)
    import train as tr
    from utils import AttrDict, get_config
    cfg = AttrDict(dict(get_config()))
    assert "speaker_heads" not in (cfg.get("runtime", {}) or {})           # the shipped default: absent = off
    assert tr.speaker_heads_settings(cfg) is None
    with_heads = lambda **kw: AttrDict(dict(cfg, runtime=AttrDict(dict(cfg.runtime, **kw))))          # noqa: E731
    assert tr.speaker_heads_settings(with_heads(speaker_heads=AttrDict(same=1, other=2))) == (1, 2)
    assert tr.speaker_heads_settings(with_heads(speaker_heads=AttrDict(same=2))) == (2, 0)
    assert tr.speaker_heads_settings(with_heads(speaker_heads=None)) is None
    for bad in (AttrDict(same=0, other=0), AttrDict(same=-1, other=1), AttrDict(same=1, others=1), 3, AttrDict(same=1.5)):
        with pytest.raises(ValueError, match="runtime.speaker_heads"):
            tr.speaker_heads_settings(with_heads(speaker_heads=bad))
    with pytest.raises(ValueError, match="device_batcher"):
        tr.speaker_heads_settings(with_heads(speaker_heads=AttrDict(same=1, other=1), device_batcher=True))
    with pytest.raises(ValueError, match="single process"):
        tr.speaker_heads_settings(with_heads(speaker_heads=AttrDict(same=1, other=1)), world=2)

    class _M:
        speaker_heads = (1, 1)
    assert tr._speaker_kw(object(), {}, "cpu") == {}
    kw = tr._speaker_kw(_M(), {"speaker": torch.ones(1, 2, dtype=torch.int64)}, "cpu")
    assert kw["speakers"].tolist() == [[1, 1]] and kw["speakers"].dtype == torch.uint8          # (checked and narrowed on the host)
    with pytest.raises(ValueError, match="0 .. 255"):
        tr._speaker_kw(_M(), {"speaker": torch.full((1, 2), 300)}, "cpu")
    with pytest.raises(ValueError, match="speaker"):
        tr._speaker_kw(_M(), {}, "cpu")


# ---- the snapshot's field ------------------------------------------------------------------------------------------------------------
SITES = ((2, 8), (4, 4))


def _snap(ring=None, lengths=(0, 1, 4, 5, 7, 13, 2), with_speakers=True):
    C = ring or 16
    rows = streaming.snapshot_rows(lengths, ring)
    sig = streaming.make_signature(SITES, False, None if ring is None else ring - 1, C)
    W = streaming.snapshot_row_elems(SITES, False)
    g = torch.Generator().manual_seed(5)
    data = torch.randn(sum(rows) * W, generator=g)
    spk = torch.randint(0, 256, (sum(rows),), generator=g).to(torch.uint8) if with_speakers else None
    return StreamSnapshot(data, lengths, streaming.snapshot_row_offsets(rows), sig, speakers=spk), rows


@pytest.mark.parametrize("ring", [None, 5])
def test_snapshot_carries_speakers(ring):
    snap, rows = _snap(ring)
    assert snap.speakers.numel() == sum(rows)
    pick = [5, 0, 2, 2]
    sel = snap.select(pick)
    want = torch.cat([snap.speakers[snap.row_offsets[i]: snap.row_offsets[i] + rows[i]] for i in pick])
    assert torch.equal(sel.speakers, want) and sel.lengths == [snap.lengths[i] for i in pick]
    for moved in (snap.cpu(), snap.to("cpu"), StreamSnapshot.from_state_dict(snap.state_dict())):
        assert torch.equal(moved.speakers, snap.speakers) and torch.equal(moved.data, snap.data) and moved.signature == snap.signature
    plain, _ = _snap(ring, with_speakers=False)
    assert plain.speakers is None and "speakers" not in plain.state_dict() and plain.select([1, 2]).speakers is None
    assert StreamSnapshot.from_state_dict(plain.state_dict()).speakers is None
    for bad in (snap.speakers[:-1], snap.speakers.to(torch.int64), snap.speakers.view(1, -1)):
        with pytest.raises(ValueError, match="speakers"):
            StreamSnapshot(snap.data, snap.lengths, snap.row_offsets, snap.signature, speakers=bad)
