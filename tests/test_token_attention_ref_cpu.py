"""Pins tests/golden/token_attention_ref.py (the float64 references tests/test_text_encoder_kernels_gpu.py holds the fp32 token attention
and embedding LayerNorm kernels to) and the constructed inputs of tests/golden/token_attention_cases.py, without a GPU."""
import pytest
import torch

import synth_roberta as SR
import token_attention_cases as TC
import token_attention_ref as TR
from oracle import roberta_oracle as RO


def _sdpa(q, k, v, kp, H):
    B, S, E = q.shape
    hd = E // H
    qh, kh, vh = (t.double().view(B, S, H, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    mask = None if kp is None else ~kp.bool()[:, None, None, :].expand(B, H, S, S)
    out = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask)
    return out.permute(0, 2, 1, 3).reshape(B, S, E)


@pytest.mark.parametrize("B,S,H,hd,mask", [(2, 19, 3, 8, "none"), (2, 70, 2, 25, "ragged"), (2, 131, 2, 16, "holes"), (2, 130, 2, 12, "lead64"),
                                           (1, 1, 2, 64, "none")])
def test_attention_reference_is_torchs_sdpa_in_float64(B, S, H, hd, mask):
    g = torch.Generator().manual_seed(S + hd)
    q, k, v = (torch.randn(B, S, H * hd, generator=g) for _ in range(3))
    kp = TC.key_pad(TC.AttnCase(B, S, H, hd, "packed", mask, "randn"))
    if mask == "lead64":
        assert kp[0, :64].all() and not kp[0, 64:].any()                   # a fully padded leading block, live blocks behind it
    out, top = TR.token_attention(q, k, v, kp, H)
    assert out.dtype == torch.float64 and (out - _sdpa(q, k, v, kp, H)).abs().max().item() < 1e-12
    live = torch.ones(B, S, dtype=torch.bool) if kp is None else ~kp.bool()
    sc = TR.scores(q, k, H)
    want = max(sc[b][:, live[b]][:, :, live[b]].abs().max().item() for b in range(B))
    assert top == want


def test_attention_reference_gives_zero_rows_where_every_key_is_padded():
    c = TC.AttnCase(3, 130, 2, 12, "packed", "lead64+dead", "randn")
    (q, k, v), kp = TC.attn_inputs(c)
    assert kp[1].all() and kp[0, :64].all() and not kp[0, 64:].any()
    out, _ = TR.token_attention(q, k, v, kp, c.H)
    assert torch.isfinite(out).all() and out[1].abs().max().item() == 0.0
    keep = torch.tensor([0, 2])
    ref = _sdpa(q[keep], k[keep], v[keep], kp[keep], c.H)                   # the other sequences: torch's numbers, dead one or not
    assert (out[keep] - ref).abs().max().item() < 1e-9 * ref.abs().max().item()


def test_embedding_reference_is_the_oracles_embeddings():
    c, B, S, lengths = SR.CASES["roberta_tiny"]
    sd = {n: t.double() for n, t in SR.make_state_dict(c).items()}
    ids, _ = SR.make_batch(c, B, S, lengths)
    want = RO.embeddings(sd, ids, c["pad_token_id"], c["layer_norm_eps"])
    pos = RO.position_ids(ids, c["pad_token_id"])
    sd32 = SR.make_state_dict(c)
    got = TR.embed_layernorm(ids.reshape(-1), pos.reshape(-1), sd32["embeddings.word_embeddings.weight"], sd32["embeddings.position_embeddings.weight"],
                             sd32["embeddings.token_type_embeddings.weight"][0], sd32["embeddings.LayerNorm.weight"], sd32["embeddings.LayerNorm.bias"],
                             c["layer_norm_eps"])
    assert got.dtype == torch.float64 and (got.view(B, S, -1) - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("c", [c for c in TC.ATTN_CASES if c.family != "randn"], ids=TC.case_id)
def test_large_score_inputs_stay_inside_their_stated_condition(c):
    (q, k, v), kp = TC.attn_inputs(c)
    _, top = TR.token_attention(q, k, v, kp, c.H)
    assert 10.0 <= top <= TC.SCORE_CAP, top                                # "in the tens", exp far from overflow after the max is taken off
    if c.family == "sharp":
        assert abs(top - TC.SHARP_TARGET) < 0.01
        return
    assert kp is None
    sc = TR.scores(q, k, c.H)
    bmax = torch.stack([sc[..., j: j + 64].max(-1).values for j in range(0, c.S, 64)], -1)      # [B, H, S, key blocks]
    assert bmax.shape[-1] == 4
    step = bmax[..., 1:] - bmax[..., :-1]
    if c.family == "rising":
        assert (step > 1.0).all()                                          # alpha < 1 in every block, for every query
    else:
        assert (step < -1.0).all()                                         # the maximum never rises behind block 0
        assert (sc.argmax(-1) < 64).all()


@pytest.mark.parametrize("c", [c for c in TC.ATTN_CASES if c.mask != "none"], ids=TC.case_id)
def test_padded_rows_hold_large_finite_values_and_padded_queries_are_saturated(c):
    (q, k, v), kp = TC.attn_inputs(c)
    pad = kp.bool()
    assert pad.any() and all(torch.isfinite(t).all() for t in (q, k, v))
    for t in (q, k, v):
        assert t[pad].abs().mean().item() > 0.5 * TC.PAD_VALUE and t[~pad].abs().max().item() < 100.0
    sc = TR.scores(q, k, c.H).masked_fill(pad[:, None, None, :], float("-inf"))
    if c.S >= 2:
        top2 = sc.topk(2, dim=-1).values
        gap = (top2[..., 0] - top2[..., 1]).permute(0, 2, 1)[pad]           # [padded queries, H]
        assert not (gap < TC.PAD_GAP).any()


def test_the_masks_are_what_their_names_say():
    for c in TC.ATTN_CASES:
        kp = TC.key_pad(c)
        if c.mask == "none":
            assert kp is None
            continue
        assert kp.shape == (c.B, c.S) and kp.any()
        dead = [b for b in range(c.B) if kp[b].all()]
        assert dead == ([1] if "dead" in c.mask else [])
        if "lead64" in c.mask:
            assert kp[0, :64].all() and not kp[0, 64:].any() and c.S > 64
        if c.mask == "holes":
            assert not kp[:, 0].any() and not kp[:, -1].any() and (kp[:, 1:-1].sum(1) > 0).all()
        if c.mask == "ragged":
            for b in range(c.B):
                n = int((kp[b] == 0).sum())
                assert 1 <= n < c.S and not kp[b, :n].any() and kp[b, n:].all()


def test_embedding_inputs_reach_the_table_edges_and_the_offset_rows_are_ill_conditioned():
    for d, T, data in TC.EMBED_CASES:
        ids, pos_ids, word, pos, type_row0, gamma, beta = TC.embed_inputs(d, T, data)
        assert ids.max().item() == TC.EMBED_VOCAB - 1 and pos_ids.max().item() == TC.EMBED_MAX_POS - 1
        if T >= 5:
            assert ids.min().item() == 0 and len(set(ids.tolist())) < T and (pos_ids == TC.EMBED_PAD_ID).any()
        if data == "offset":
            x = word.double()[ids] + pos.double()[pos_ids] + type_row0.double()
            assert (x.mean(-1).abs() > 100.0 * x.std(-1)).all()
