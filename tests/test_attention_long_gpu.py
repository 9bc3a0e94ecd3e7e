"""Long-dialogue attention kernels (attention_dlong.hip, m2f_attention_varlen_fwd / _bwd) against torch float64 math on the same
tensors: packed (cu) and padded (key_pad) rows, strided column-slice operands, odd head dims, dropout replay, run-to-run bits,
and agreement with the L <= 64 dialogue kernels."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402

DEV = "cuda"


def _lengths(B, L):
    base = [L, 1, L // 2 + 3, 7, L - 1]
    return [max(1, min(L, n)) for n in base[:B]]


def _case(L, hd, H, packed, seed):
    """q / k / v as column slices of one wide buffer (v at an odd column offset), rows of B ragged dialogues."""
    B = 4
    lens = _lengths(B, L)
    g = torch.Generator(device="cpu").manual_seed(seed)
    E = H * hd
    if packed:
        cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)
        T = int(cu[-1]) + 5                                   # 5 rows behind the last dialogue
        rows = [(int(cu[b]), lens[b]) for b in range(B)]
        kp = None
    else:
        cu, T = None, B * L
        rows = [(b * L, L) for b in range(B)]
        kp = torch.ones(B, L, dtype=torch.bool)
        for b, n in enumerate(lens):
            kp[b, :n] = False
    wide = torch.randn(T, 3 * E + 3, generator=g) * 0.7
    q, k, v = wide[:, :E], wide[:, E:2 * E], wide[:, 2 * E + 3:]
    dout = torch.randn(T, E, generator=g)
    dev = lambda t: None if t is None else t.to(DEV)        # noqa: E731
    wide_d = wide.to(DEV)
    qd, kd, vd = wide_d[:, :E], wide_d[:, E:2 * E], wide_d[:, 2 * E + 3:]
    return dict(B=B, L=L, H=H, hd=hd, T=T, rows=rows, cu=dev(cu), kp=dev(kp), kp_cpu=kp, q=q, k=k, v=v, dout=dout,
                qd=qd, kd=kd, vd=vd, doutd=dout.to(DEV))


def _reference(c, keep=None, p=0.0):
    """float64 autograd per (dialogue, head): (out, P [B, H, L, L], dq, dk, dv); keep: [B, H, L, L] dropout mask."""
    H, hd, L = c["H"], c["hd"], c["L"]
    q, k, v = (t.double().to(DEV).requires_grad_(True) for t in (c["q"], c["k"], c["v"]))
    out = torch.zeros(c["T"], H * hd, dtype=torch.float64, device=DEV)
    P = torch.zeros(c["B"], H, L, L, dtype=torch.float64, device=DEV)
    outs = []
    for b, (r0, n) in enumerate(c["rows"]):
        for h in range(H):
            cs = slice(h * hd, (h + 1) * hd)
            s = q[r0:r0 + n, cs] @ k[r0:r0 + n, cs].T / math.sqrt(hd)
            if c["kp_cpu"] is not None:
                s = s.masked_fill(c["kp_cpu"][b, :n].to(DEV)[None, :], float("-inf"))
            pr = torch.softmax(s, dim=-1)
            P[b, h, :n, :n] = pr.detach()
            if keep is not None:
                pr = pr * keep[b, h, :n, :n].double() / (1 - p)
            outs.append((r0, n, cs, pr @ v[r0:r0 + n, cs]))
    for r0, n, cs, o in outs:
        out = out.index_put((torch.arange(r0, r0 + n, device=DEV)[:, None], torch.arange(cs.start, cs.stop, device=DEV)[None, :]), o)
    out.backward(c["dout"].double().to(DEV))
    return out.detach(), P, q.grad, k.grad, v.grad


def _close(got, ref, tol, what):
    if got.numel() == 0:
        return
    err = (got.double() - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1.0)
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e})"


def _run(c, drop_site=0, p=0.0, rng=None, v=None):
    vd = c["vd"] if v is None else v
    kw = dict(cu=c["cu"], key_pad=c["kp"], drop_site=drop_site, drop_p=p, rng=rng)
    out, probs = F.attention_varlen_fwd(c["qd"], c["kd"], vd, c["B"], c["L"], c["H"], **kw)
    dq, dk, dv = F.attention_varlen_bwd(c["qd"], c["kd"], vd, out, probs, c["doutd"], c["B"], c["L"], c["H"], **kw)
    return out, probs, dq, dk, dv


def _probs_view(c, probs):
    Lp = probs.shape[-1]
    return probs.view(c["B"], c["H"], Lp, Lp)[:, :, :c["L"], :c["L"]].transpose(-1, -2)


def _live(c):
    """rows of the result the kernels own: every row of a padded batch, the dialogues' rows of a packed one"""
    m = torch.zeros(c["T"], dtype=torch.bool, device=DEV)
    for r0, n in c["rows"]:
        m[r0:r0 + n] = True
    return m


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("hd", [25, 60, 96, 128, 256])
@pytest.mark.parametrize("L", [65, 96, 110, 128, 129, 200, 512])
def test_varlen_forward_backward_against_float64(L, hd, packed):
    H = 2 if hd >= 96 else 3
    c = _case(L, hd, H, packed, seed=L * 7 + hd)
    out, probs, dq, dk, dv = _run(c)
    ro, rP, rdq, rdk, rdv = _reference(c)
    live = _live(c)
    _close(out[live], ro[live], 2e-5, "out")
    P = _probs_view(c, probs)
    for b, (r0, n) in enumerate(c["rows"]):
        _close(P[b, :, :n, :n], rP[b, :, :n, :n], 2e-5, f"probs of dialogue {b}")
    for name, g, r in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        _close(g[live], r[live], 5e-5, name)
    if packed:                                                # rows behind the last dialogue: zeros
        tail = ~live
        for t in (out, dq, dk, dv):
            assert torch.all(t[tail] == 0)


def test_varlen_runs_are_bit_identical():
    c = _case(200, 60, 3, True, seed=3)
    rng = torch.tensor([5, 6, 7, 0], dtype=torch.int32, device=DEV)
    a = _run(c, drop_site=4, p=0.2, rng=rng)
    b = _run(c, drop_site=4, p=0.2, rng=rng)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "padded"])
@pytest.mark.parametrize("L", [65, 129, 256])
def test_varlen_dropout_backward_matches_autograd_with_same_mask(L, packed):
    """H = 1, hd = 256 >= L: V = [I | 0] per dialogue exposes the dropped probabilities in the output."""
    p, hd, H = 0.3, 256, 1
    c = _case(L, hd, H, packed, seed=L)
    rng = torch.tensor([9, 8, 3, 0], dtype=torch.int32, device=DEV)
    eye = torch.zeros(c["T"], hd, device=DEV)
    for r0, n in c["rows"]:
        eye[r0:r0 + n, :n] = torch.eye(n, device=DEV)
    out, probs = F.attention_varlen_fwd(c["qd"], c["kd"], eye, c["B"], L, H, cu=c["cu"], key_pad=c["kp"], drop_site=3, drop_p=p, rng=rng)
    P = _probs_view(c, probs)
    keep = torch.zeros(c["B"], H, L, L, dtype=torch.bool, device=DEV)
    for b, (r0, n) in enumerate(c["rows"]):
        Pd = out[r0:r0 + n, :n]
        keep[b, 0, :n, :n] = Pd != 0
        live = P[b, 0, :n, :n] > 1e-12
        _close(Pd[keep[b, 0, :n, :n]], (P[b, 0, :n, :n] / (1 - p))[keep[b, 0, :n, :n]], 1e-5, "dropped probs scaled")
        if live.sum() > 200:
            rate = keep[b, 0, :n, :n][live].float().mean().item()
            assert abs(rate - (1 - p)) < 0.08, rate
    o, probs2, dq, dk, dv = _run(c, drop_site=3, p=p, rng=rng)
    ro, _, rdq, rdk, rdv = _reference(c, keep=keep, p=p)
    live = _live(c)
    _close(o[live], ro[live], 2e-5, "dropout forward")
    for name, g, r in (("dq", dq, rdq), ("dk", dk, rdk), ("dv", dv, rdv)):
        _close(g[live], r[live], 5e-5, name)


@pytest.mark.parametrize("L,hd", [(16, 32), (33, 25), (64, 128), (48, 160)])
def test_varlen_agrees_with_dialogue_kernels_up_to_64(L, hd):
    H = 2
    c = _case(L, hd, H, False, seed=L + hd)
    kp_flat = c["kp"].reshape(-1)
    out_s, probs_s = F.attention_fwd(c["qd"], c["kd"], c["vd"], kp_flat, c["B"], L, H)
    dq_s, dk_s, dv_s = F.attention_bwd(c["qd"], c["kd"], c["vd"], kp_flat, out_s, probs_s, c["doutd"], c["B"], L, H)
    out, probs, dq, dk, dv = _run(c)
    for a, b_, what in ((out, out_s, "out"), (dq, dq_s, "dq"), (dk, dk_s, "dk"), (dv, dv_s, "dv")):
        _close(a, b_.double(), 3e-5, what)
    _close(_probs_view(c, probs), _probs_view(c, probs_s).double(), 2e-5, "probs")
