"""Bits of the row-wise kernels (LayerNorm forward / backward, dialogue attention, criterion, row dropout) and of one bf16 train
step, recorded from a build on an MI355X:  python3 tests/golden/make_rowwise_parent_bits.py  ->  tests/golden/rowwise_parent_bits.npz

tests/test_rowwise_loads_gpu.py runs compute() on the build under test and asks for the same bits.  The file was recorded from the
build in front of the change that batched these kernels' loads (no arithmetic changed, so no bit may); re-record it only with a
change that is meant to move results.

Every input comes from a seeded CPU generator.  Every output is kept as raw bits (uint32 / uint16 / uint8 views), so NaNs and signed
zeros compare like any other value.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(HERE, "rowwise_parent_bits.npz")
DEV = "cuda"
STATE = [123, 456, 7, 0]
P_DROP = 0.4
T_LN = 5

# LayerNorm: (d, ld, residual / extra, dropout site, x offset by 4 bytes).  T = 5: the second row block is partly filled.
#   768 under NV = 3, 1024 under NV = 4, 300 with a partly filled chunk: the 16-byte path; 301 and the offset pointer: the general path
LN_CASES = {
    "ln768": (768, 768, True, 0, False),
    "ln768_ld_site": (768, 772, False, 4, False),
    "ln1024_site": (1024, 1024, True, 4, False),
    "ln300_ld": (300, 304, True, 0, False),
    "ln301_site": (301, 301, True, 4, False),
    "ln300_offset": (300, 300, False, 4, True),
}
# attention through m2f_attention_fwd / _bwd: (L, hd, lengths, dropout site, M2F_ATTN_BF16_KERNEL form); B = 3, H = 2
ATTN_CASES = {
    "attn_L16_hd128_drop": (16, 128, [16, 1, 9], 4, 0),
    "attn_L5_hd60": (5, 60, [3, 5, 1], 0, 0),
    "attn_L5_hd96_drop_bf16math": (5, 96, [5, 1, 3], 4, 1),
    "attn_L5_hd60_drop_bf16shadows": (5, 60, [2, 5, 4], 4, 63),
    "attn_L1_hd128": (1, 128, [1, 1, 1], 0, 0),
}
# the varlen forms: (L, hd, lengths, dropout site, packed rows, token rows left behind the last dialogue)
VARLEN_CASES = {
    "varlen_packed_L5_hd96_drop": (5, 96, [5, 1, 3], 6, True, 3),
    "varlen_padded_L5_hd60": (5, 60, [4, 5, 1], 0, False, 0),
    "varlen_packed_L16_hd60": (16, 60, [16, 2, 11], 0, True, 2),
}
B_ATT, H_ATT = 3, 2


def rng_tensor(state=STATE):
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in state], dtype=torch.int32, device=DEV)


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    """raw bits of a tensor as a numpy array of unsigned integers"""
    t = t.detach().contiguous().cpu()
    view = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()]
    a = t.view(view).numpy()
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[t.element_size()]).copy()


def rows(t, ld, offset=False, fill=9.0):
    """[T, d] values as rows of stride ld on the device (pad columns hold a sentinel), optionally starting 4 bytes past a 16-byte boundary"""
    T, d = t.shape
    flat = torch.full((T * ld + 4,), fill)
    o = 1 if offset else 0
    flat[o: o + T * ld].view(T, ld)[:, :d] = t
    return flat.to(DEV)[o: o + T * ld].view(T, ld)[:, :d]


def ln_inputs(d, seed=60):
    T = T_LN
    return dict(x=rand(T, d, seed=seed, scale=3.0), g=1 + 0.1 * rand(d, seed=seed + 1), b=0.1 * rand(d, seed=seed + 2),
                res=rand(T, d, seed=seed + 3), dy=rand(T, d, seed=seed + 4), extra=rand(T, d, seed=seed + 5))


def ln_run(d, ld, with_res, site, offset):
    """forward (site) and backward (extra, masked second output at site + 4) of one LayerNorm; every buffer has row stride ld"""
    from mer_amd import runtime
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    i = ln_inputs(d)
    x, res, dy, extra = (rows(i[k], ld, offset) for k in ("x", "res", "dy", "extra"))
    g, b = i["g"].to(DEV), i["b"].to(DEV)
    out, dx, dxm = (rows(torch.zeros(T_LN, d), ld, offset) for _ in range(3))
    stats = torch.zeros(T_LN, 2, device=DEV)
    partial = torch.zeros((T_LN + 3) // 4, 2, d, device=DEV)
    dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    rng = rng_tensor()
    check(lib().m2f_layernorm_fwd_drop(T_LN, d, ld, ptr(x), ptr(g), ptr(b), ptr(res) if with_res else None, ptr(out), ptr(stats), 1e-5,
                                       site, P_DROP if site else 0.0, ptr(rng) if site else None, stream_ptr()), "m2f_layernorm_fwd_drop")
    site2 = site + 4 if site else 0
    check(lib().m2f_layernorm_bwd_masked(T_LN, d, ld, ptr(x), ptr(g), ptr(stats), ptr(dy), ptr(extra) if with_res else None, ptr(dx),
                                         ptr(dxm), ptr(partial), ptr(dg), ptr(db), site2, P_DROP if site2 else 0.0,
                                         ptr(rng) if site2 else None, stream_ptr()), "m2f_layernorm_bwd_masked")
    torch.cuda.synchronize()
    return dict(out=out, stats=stats, dx=dx, dxm=dxm, dg=dg, db=db)


def ln_plain(d):
    """m2f_layernorm_fwd / m2f_layernorm_bwd (contiguous rows, no site), with and without the residual / extra term"""
    from mer_amd import functional as F
    i = {k: v.to(DEV) for k, v in ln_inputs(d, seed=80).items()}
    r = {}
    for tag, res, extra in (("res", i["res"], i["extra"]), ("nores", None, None)):
        out, stats = F.layernorm_fwd(i["x"], i["g"], i["b"], res)
        dx, dg, db = F.layernorm_bwd(i["x"], i["g"], stats, i["dy"], extra)
        r.update({f"{tag}.out": out, f"{tag}.stats": stats, f"{tag}.dx": dx, f"{tag}.dg": dg, f"{tag}.db": db})
    torch.cuda.synchronize()
    return r


def ln_shadowed(d=768):
    """forward whose result lies inside a shadowed workspace: the fp32 rows and their bf16 copies"""
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    i = {k: v.to(DEV) for k, v in ln_inputs(d, seed=90).items()}
    ws = torch.zeros(T_LN, d, device=DEV)
    sh = torch.zeros(T_LN, d, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(T_LN, 2, device=DEV)
    check(lib().m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        check(lib().m2f_layernorm_fwd_drop(T_LN, d, d, ptr(i["x"]), ptr(i["g"]), ptr(i["b"]), ptr(i["res"]), ptr(ws), ptr(stats), 1e-5, 4,
                                           P_DROP, ptr(rng_tensor()), stream_ptr()), "m2f_layernorm_fwd_drop")
        torch.cuda.synchronize()
    finally:
        check(lib().m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
    return dict(out=ws, out16=sh, stats=stats)


def ln_two_problems():
    """m2f_layernorm_fwd_diag: d = 768 and d = 1024 in one launch (the kernel instantiated for the wider one serves both)"""
    import ctypes
    from mer_amd.runtime import check, lib, stream_ptr
    ds = [768, 1024]
    ins = [{k: v.to(DEV) for k, v in ln_inputs(d, seed=100 + n).items()} for n, d in enumerate(ds)]
    outs = [torch.zeros(T_LN, d, device=DEV) for d in ds]
    stats = [torch.zeros(T_LN, 2, device=DEV) for _ in ds]
    arr = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])          # noqa: E731
    check(lib().m2f_layernorm_fwd_diag(T_LN, 2, (ctypes.c_int * 2)(*ds), arr([i["x"] for i in ins]), arr([i["g"] for i in ins]),
                                       arr([i["b"] for i in ins]), arr(outs), arr(stats), 1e-5, 0, stream_ptr()), "m2f_layernorm_fwd_diag")
    torch.cuda.synchronize()
    return {"out0": outs[0], "out1": outs[1], "stats0": stats[0], "stats1": stats[1]}


def attn_inputs(L, hd, lengths, seed):
    E, T = H_ATT * hd, B_ATT * L
    q, k, v, dout = (rand(T, E, seed=seed + n, scale=0.5) for n in range(4))
    key_pad = torch.zeros(B_ATT, L, dtype=torch.bool)
    for b, n in enumerate(lengths):
        key_pad[b, n:] = True
    return q, k, v, dout, key_pad


def attn_run(L, hd, lengths, site, form):
    """forward and backward of the dialogue kernels; every operand and result is a column block of one workspace that has a bf16
    shadow (the bf16 forms stage from it, and every result is also written into it)"""
    from mer_amd.runtime import check, lib, ptr, stream_ptr
    E, T = H_ATT * hd, B_ATT * L
    ld = (3 * E + 7) // 8 * 8
    q, k, v, dout, key_pad = attn_inputs(L, hd, lengths, seed=40 + L + hd)
    ws = torch.zeros(3 * T, ld)
    ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:2 * T, :E] = q, k, v, dout
    ws = ws.to(DEV)
    sh = ws.to(torch.bfloat16).contiguous()
    kp = key_pad.reshape(-1).to(torch.uint8).to(DEV)
    Lp = 16 * ((L + 15) // 16)
    probs = torch.zeros(B_ATT * H_ATT, Lp, Lp, device=DEV)
    qd, kd, vd, dd = ws[:T, :E], ws[:T, E:2 * E], ws[:T, 2 * E:3 * E], ws[T:2 * T, :E]
    out, dq, dk, dv = ws[T:2 * T, E:2 * E], ws[T:2 * T, 2 * E:3 * E], ws[2 * T:, :E], ws[2 * T:, E:2 * E]
    rng = rng_tensor()
    old = os.environ.get("M2F_ATTN_BF16_KERNEL")
    os.environ["M2F_ATTN_BF16_KERNEL"] = str(form)
    check(lib().m2f_set_shadow_map(ws.data_ptr(), sh.data_ptr(), ws.numel()), "m2f_set_shadow_map")
    try:
        check(lib().m2f_attention_fwd(B_ATT, L, H_ATT, hd, ptr(qd), ld, ptr(kd), ld, ptr(vd), ld, ptr(kp), ptr(out), ld, ptr(probs), site,
                                      P_DROP if site else 0.0, ptr(rng) if site else None, stream_ptr(), None), "m2f_attention_fwd")
        check(lib().m2f_attention_bwd(B_ATT, L, H_ATT, hd, ptr(qd), ld, ptr(kd), ld, ptr(vd), ld, ptr(kp), ptr(out), ld, ptr(probs), ptr(dd),
                                      ld, ptr(dq), ld, ptr(dk), ld, ptr(dv), ld, site, P_DROP if site else 0.0, ptr(rng) if site else None,
                                      stream_ptr(), -1, -1), "m2f_attention_bwd")
        torch.cuda.synchronize()
    finally:
        check(lib().m2f_set_shadow_map(None, None, 0), "m2f_set_shadow_map")
        if old is None:
            os.environ.pop("M2F_ATTN_BF16_KERNEL", None)
        else:
            os.environ["M2F_ATTN_BF16_KERNEL"] = old
    # results only (the operands' columns of the workspace are inputs): out | dq, dk | dv, and their shadows (kept for the bf16 forms
    # only, to hold the fixture's size down; the fp32 forms write them through the same statements)
    r = dict(probs=probs, res1=ws[T:2 * T, E:3 * E], res2=ws[2 * T:, :2 * E])
    if form:
        r.update(res1_16=sh[T:2 * T, E:3 * E], res2_16=sh[2 * T:, :2 * E])
    return r


def varlen_run(L, hd, lengths, site, packed, tail):
    from mer_amd import functional as F
    q, k, v, dout, key_pad = attn_inputs(L, hd, lengths, seed=70 + L + hd)
    valid = ~key_pad.reshape(-1)
    if packed:
        idx = valid.nonzero()[:, 0]
        pad_rows = lambda t: torch.cat([t[idx], torch.full((tail, t.shape[1]), 7.0)])          # noqa: E731
        qd, kd, vd, dd = (pad_rows(t).to(DEV) for t in (q, k, v, dout))
        kw = dict(cu=torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=DEV))
    else:
        qd, kd, vd, dd = (t.to(DEV) for t in (q, k, v, dout))
        kw = dict(key_pad=key_pad.to(DEV))
    if site:
        kw.update(drop_site=site, drop_p=P_DROP, rng=rng_tensor())
    out, probs = F.attention_varlen_fwd(qd, kd, vd, B_ATT, L, H_ATT, **kw)
    dq, dk, dv = F.attention_varlen_bwd(qd, kd, vd, out, probs, dd, B_ATT, L, H_ATT, **kw)
    torch.cuda.synchronize()
    return dict(out=out, probs=probs, dq=dq, dk=dk, dv=dv)


def ce_run():
    from mer_amd import functional as F
    r = {}
    for tag, T, C, weighted in (("c7w", 37, 7, True), ("c16", 300, 16, False)):
        logits = rand(T, C, seed=120 + C, scale=2.0).to(DEV)
        labels = torch.randint(-1, C, (T,), generator=torch.Generator().manual_seed(130 + C)).to(DEV)
        w = (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(140))).to(DEV) if weighted else None
        out, dl = F.cross_entropy(logits, labels, w, 0.1, True)
        r[f"{tag}.loss"], r[f"{tag}.dlogits"] = out, dl
    torch.cuda.synchronize()
    return r


def dropout_rows_run():
    from mer_amd import functional as F
    a, b = rows(rand(T_LN, 300, seed=150), 304), rows(rand(T_LN, 300, seed=151), 304)
    F.dropout_rows(a, 4, P_DROP, rng_tensor(), x2=b, site2=8)
    c = rows(rand(33, 50, seed=152), 50)
    F.dropout_rows(c, 12, P_DROP, rng_tensor())
    torch.cuda.synchronize()
    return dict(a=a, b=b, c=c)


def train_step_run():
    """forward / loss / backward of the bf16 train plan of synth's tiny_ragged case, dropout 0.4, at a fixed rng state"""
    import synth
    import mer_amd  # noqa: F401
    from mer_amd.model import M2FNet
    cfg, B, L, lengths, _ = synth.CASES["tiny_ragged"]
    cfg = dict(cfg, dropout=P_DROP)
    sd = synth.make_state_dict(cfg)
    batch = synth.make_inputs(cfg, B, L, lengths, "randn")
    torch.manual_seed(20261017)                    # the engine seeds its rng from torch's seed
    m = M2FNet(cfg, precision="bf16")
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    eng = m.engine()
    plan = eng.plan(B, L, True, True, None, (0, True))
    plan.set_inputs(*[t.cuda() for t in batch])
    plan.forward()
    loss = plan.loss_fwd(0.1, False, True)[0]
    plan.backward()
    torch.cuda.synchronize()
    return dict(rng=eng.rng, logits=plan.logits, loss=loss.reshape(1), **digest("grad", eng.flat_grad))


def digest(name, t, chunk=1024):
    """A buffer too large to keep (the flat gradient: a million elements): the SHA-256 of its bits - equal digests, equal bits - and,
    to point at what moved, the wrapping sum and the xor of the bits of every `chunk` elements."""
    import hashlib
    a = bits(t).reshape(-1)
    pad = np.zeros((-a.size) % chunk, dtype=a.dtype)
    c = np.concatenate([a, pad]).reshape(-1, chunk)
    sums = np.stack([c.sum(axis=1, dtype=np.uint64), np.bitwise_xor.reduce(c, axis=1).astype(np.uint64)], axis=1)
    return {f"{name}_sha256": np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy(), f"{name}_chunks": sums,
            f"{name}_numel": np.array([a.size], dtype=np.uint64)}


GROUPS = {}
for _name, _c in LN_CASES.items():
    GROUPS[_name] = (lambda c=_c: ln_run(*c))
GROUPS["ln_plain300"] = lambda: ln_plain(300)
GROUPS["ln_shadowed"] = ln_shadowed
GROUPS["ln_two_problems"] = ln_two_problems
for _name, _c in ATTN_CASES.items():
    GROUPS[_name] = (lambda c=_c: attn_run(*c))
for _name, _c in VARLEN_CASES.items():
    GROUPS[_name] = (lambda c=_c: varlen_run(*c))
GROUPS["ce"] = ce_run
GROUPS["dropout_rows"] = dropout_rows_run
GROUPS["train_step"] = train_step_run


def compute(group):
    """{'<group>/<output>': bits} of one group on the build that mer_amd loads"""
    return {f"{group}/{k}": v if isinstance(v, np.ndarray) else bits(v) for k, v in GROUPS[group]().items()}


if __name__ == "__main__":
    import mer_amd  # noqa: F401
    rec = {}
    for name in GROUPS:
        rec.update(compute(name))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} arrays, {sum(a.nbytes for a in rec.values())} bytes raw, {os.path.getsize(out)} bytes on disk -> {out}")
    print("train_step grad elements:", int(rec["train_step/grad_numel"][0]))
