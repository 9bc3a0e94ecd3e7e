"""Bits of the one-tile dialogue attention kernels (forward and backward, the ones a training step launches), recorded on an MI355X from
the build in front of the change that made their result stores write-through:
    python3 tests/golden/make_chain_store_parent_bits.py  ->  tests/golden/chain_store_parent_bits.npz

tests/test_chain_stores_gpu.py runs compute() on the build under test and asks for the same bits: the store policy moves no value.
Re-record only with a change that is meant to move results.  Inputs come from seeded CPU generators (make_rowwise_parent_bits.rand);
outputs are kept as raw bits.

Cases: B = 2, H = 2, L in {5, 16}, head dim in {32, 96}; ragged lengths; the L = 16 cases with attention dropout.  Every result - out,
probs, dq, dk, dv - and every bf16 shadow is recorded, and so is the rest of the workspace around them: a store that strays shows."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import make_rowwise_parent_bits as G  # noqa: E402

FIXTURE = os.path.join(HERE, "chain_store_parent_bits.npz")
B, H = 2, 2
# name: (L, head dim, lengths, dropout site)
CASES = {
    "attn_L5_hd32": (5, 32, [5, 3], 0),
    "attn_L5_hd96": (5, 96, [2, 5], 0),
    "attn_L16_hd32_drop": (16, 32, [16, 7], 4),
    "attn_L16_hd96_drop": (16, 96, [11, 16], 4),
}
SENTINEL = 5.0


def attn_run(L, hd, lengths, site):
    """forward and backward through m2f_attention_fwd / _bwd; operands and results are column blocks of one shadowed workspace whose
    remaining columns and rows hold a sentinel"""
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    E, T = H * hd, B * L
    ld = 3 * E + 8
    q, k, v, dout = (G.rand(T, E, seed=200 + L + hd + n, scale=0.5) for n in range(4))
    key_pad = torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    ws = torch.full((3 * T + 1, ld), SENTINEL)
    ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:2 * T, :E] = q, k, v, dout
    ws = ws.to(G.DEV)
    sh = ws.to(torch.bfloat16).contiguous()
    kp = key_pad.reshape(-1).to(torch.uint8).to(G.DEV)
    Lp = 16 * ((L + 15) // 16)
    probs = torch.full((B * H + 1, Lp, Lp), SENTINEL, device=G.DEV)
    qd, kd, vd, dd = ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:2 * T, :E]
    out, dq, dk, dv = ws[T:2 * T, E:2 * E], ws[T:2 * T, 2 * E:3 * E], ws[2 * T:3 * T, :E], ws[2 * T:3 * T, E:2 * E]
    rng = G.rng_tensor()
    check(lib().m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        check(lib().m2f_attention_fwd(B, L, H, hd, ptr(qd), ld, ptr(kd), ld, ptr(vd), ld, ptr(kp), ptr(out), ld, ptr(probs), site,
                                      G.P_DROP if site else 0.0, ptr(rng) if site else None, stream_ptr(), None), "m2f_attention_fwd")
        check(lib().m2f_attention_bwd(B, L, H, hd, ptr(qd), ld, ptr(kd), ld, ptr(vd), ld, ptr(kp), ptr(out), ld, ptr(probs), ptr(dd),
                                      ld, ptr(dq), ld, ptr(dk), ld, ptr(dv), ld, site, G.P_DROP if site else 0.0, ptr(rng) if site else None,
                                      stream_ptr(), -1, -1), "m2f_attention_bwd")
        torch.cuda.synchronize()
    finally:
        check(lib().m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
    return dict(probs=probs, ws=ws, sh=sh)


def compute(name):
    """{'<case>/<output>': bits} of one case on the build that mer_amd loads"""
    return {f"{name}/{k}": G.bits(v) for k, v in attn_run(*CASES[name]).items()}


if __name__ == "__main__":
    import mer_amd  # noqa: F401
    rec = {}
    for name in CASES:
        rec.update(compute(name))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} arrays, {sum(a.nbytes for a in rec.values())} bytes raw, {os.path.getsize(out)} bytes on disk -> {out}")
