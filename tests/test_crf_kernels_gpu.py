"""The linear-chain CRF kernels (csrc/crf.hip) against the float64 reference (tests/golden/crf_ref.py): loss, emission and parameter
gradients on padded and cu_seqlens batches, the zero-parameter case against the plain criterion, unlabelled NaN rows, forbidden
transitions and huge margins, run-to-run and batch-position bits, Viterbi and the forward filter.
Bounds (from the issue's CPU measurements of the renormalised fp32 recursion: 2.4e-7 .. 1.2e-6 in the marginals, 4e-8 .. 3e-7 in
the loss): loss 2e-6 relative, dlogits 1e-5 absolute, parameter gradient 1e-5 of its largest element.
Every comparison prints its figures before it asserts (-s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_cases as cases  # noqa: E402
import crf_ref as ref  # noqa: E402
import mer_amd  # noqa: E402,F401
from mer_amd import functional as F  # noqa: E402
from mer_amd.crf import LinearChainCRF  # noqa: E402

DEV = "cuda"
# (C, B, L, packed): every C of {2, 3, 7, 16}, B of {1, 4, 5, 257}, L of {1, 2, 17, 64, 65, 512}, both forms
NLL_CASES = [(7, 1, 1, False), (2, 4, 2, False), (3, 5, 17, True), (7, 4, 64, False), (16, 5, 65, True), (7, 5, 512, False),
             (16, 257, 17, True), (3, 257, 2, False), (7, 1, 512, True), (2, 5, 65, False), (16, 4, 1, True), (16, 4, 512, True),
             (16, 5, 512, False), (7, 257, 64, True)]
_REF = {}


def _case(key, **kw):
    """The case and its float64 reference (unnormalised gradients), computed once and shared."""
    if (key, tuple(sorted(kw.items()))) not in _REF:
        C, B, L, packed = key
        c = cases.nll_case(C, B, L, packed, seed=100 + 7 * C + 11 * B + 13 * L + int(packed), **kw)
        loss, dz, dp = ref.nll_grads(c["logits"], c["labels"], c["params"], c["spans"], normalise=False)
        num, den, _ = ref.nll(c["logits"].double(), c["labels"], c["params"], c["spans"])
        c["ref"] = {"loss": float(num) / max(den, 1), "den": den, "dz": dz, "dp": dp}
        _REF[(key, tuple(sorted(kw.items())))] = c
    return _REF[(key, tuple(sorted(kw.items())))]


def _run(c, normalise=False, param_grad=True, logits=None, params=None):
    cu = c["cu"].to(DEV) if c["cu"] is not None else None
    return F.crf_nll((c["logits"] if logits is None else logits).to(DEV), c["labels"].to(DEV),
                     (c["params"] if params is None else params).to(DEV), batch=None if cu is not None else c["B"], cu_seqlens=cu,
                     normalise=normalise, param_grad=param_grad)


def _check(c, tag):
    out, dl, dp, terms = _run(c)
    r = c["ref"]
    loss, den = float(out[0]), float(out[1])
    rel = abs(loss - r["loss"]) / max(abs(r["loss"]), 1e-30)
    e_dl = float((dl.double().cpu() - r["dz"]).abs().max())
    big = float(r["dp"].abs().max())
    e_dp = float((dp.double().cpu() - r["dp"]).abs().max()) / max(big, 1e-30)
    print(f"{tag}: loss {loss:.9g} ref {r['loss']:.9g} rel {rel:.3g} | den {den:g} ref {r['den']} | dlogits max abs err {e_dl:.3g} | "
          f"dparams max err / largest {e_dp:.3g} (largest {big:.4g})")
    assert den == r["den"]
    assert torch.isfinite(dl).all() and torch.isfinite(dp).all() and torch.isfinite(terms).all()
    assert rel <= 2e-6
    assert e_dl <= 1e-5
    assert e_dp <= 1e-5
    return out, dl, dp, terms


@pytest.mark.parametrize("key", NLL_CASES, ids=lambda k: f"C{k[0]}-B{k[1]}-L{k[2]}-{'cu' if k[3] else 'pad'}")
def test_nll_against_reference(key):
    c = _case(key)
    out, dl, dp, terms = _check(c, f"crf_nll {key}")
    # the convention of the row terms: den = 1 on chain rows, num on a dialogue's first chain row only, zeros off the chain
    lab = c["labels"]
    t = terms.cpu()
    assert torch.equal(t[:, 1], (lab >= 0).float())
    firsts = [int(rows[0]) for rows in ref.chains(lab, c["spans"]) if rows.numel()]
    other = torch.ones(c["T"], dtype=torch.bool)
    other[firsts] = False
    assert (t[other, 0] == 0).all()
    assert (dl.cpu()[lab < 0] == 0).all()


def test_normalised_outputs_and_frozen_form():
    """normalise = 1 divides dlogits and the parameter gradient by den; param_grad = False gives the same loss and dlogits bits."""
    c = _case((7, 4, 64, False))
    out0, dl0, dp0, _ = _run(c, normalise=False)
    out1, dl1, dp1, _ = _run(c, normalise=True)
    out2, dl2, dp2, _ = _run(c, normalise=True, param_grad=False)
    inv = 1.0 / out0[1]
    print("normalised: den", float(out0[1]), "max |dl1 - dl0/den|", float((dl1 - dl0 * inv).abs().max()))
    assert torch.equal(out0[:3], out1[:3]) and torch.equal(dl1, dl0 * inv) and torch.equal(dp1, dp0 * inv)
    assert dp2 is None and torch.equal(out2, out1) and torch.equal(dl2, dl1)


@pytest.mark.parametrize("key", [(7, 5, 512, False), (16, 5, 65, True), (2, 4, 2, False)], ids=str)
def test_zero_parameters_are_the_plain_criterion(key):
    c = _case(key)
    zero = torch.zeros_like(c["params"])
    out, dl, dp, _ = _run(c, normalise=True, params=zero)
    ce, dce = F.cross_entropy(c["logits"].to(DEV), c["labels"].to(DEV), None, 0.0, True)
    e_loss, e_dl = abs(float(out[0]) - float(ce[0])), float((dl - dce).abs().max())
    print(f"zero parameters {key}: loss {float(out[0]):.9g} CE {float(ce[0]):.9g} diff {e_loss:.3g} | dlogits diff {e_dl:.3g}")
    assert e_loss <= 1e-6 and e_dl <= 1e-6


@pytest.mark.parametrize("packed", [False, True], ids=["pad", "cu"])
def test_batch_without_a_label(packed):
    """No chain row anywhere: zero terms, zero dlogits and a zero parameter gradient, normalised or not (the loss itself is 0 / 0, as the
    plain criterion's); one unlabelled dialogue among labelled ones adds exact zeros."""
    c = dict(cases.nll_case(7, 5, 17, packed, seed=77))
    c["labels"] = torch.full_like(c["labels"], -1)
    for normalise in (False, True):
        out, dl, dp, terms = _run(c, normalise=normalise)
        print(f"no label, normalise {normalise}: den {float(out[1])}, num {float(out[2])}, |dparams| max {float(dp.abs().max())}")
        assert float(out[1]) == 0.0 and float(out[2]) == 0.0 and (terms == 0).all() and (dp == 0).all()
        if not normalise:
            assert (dl == 0).all()
    out, dl, dp, _ = _run(c, param_grad=False, normalise=False)
    assert dp is None and (dl == 0).all()


def test_loss_alone_has_the_train_kernels_bits():
    """logit_grad=False: the forward sweep alone (what eval_step runs) - the same loss bits, no gradient; LinearChainCRF.forward takes
    it when nothing needs a gradient."""
    c = _case((7, 4, 64, False))
    cu = None
    full = _run(c, normalise=True)
    out, dl, dp, terms = F.crf_nll(c["logits"].to(DEV), c["labels"].to(DEV), c["params"].to(DEV), batch=c["B"], cu_seqlens=cu,
                                   param_grad=False, logit_grad=False)
    assert dl is None and dp is None and torch.equal(out[:3], full[0][:3]) and torch.equal(terms, full[3])
    crf = LinearChainCRF(7).to(DEV)
    with torch.no_grad():
        crf.params.copy_(c["params"])
        loss = crf(c["logits"].view(4, 64, 7).to(DEV), c["labels"].view(4, 64).to(DEV))
    assert not loss.requires_grad and torch.equal(loss, full[0][0])
    with pytest.raises(ValueError, match="param_grad needs logit_grad"):
        F.crf_nll(c["logits"].to(DEV), c["labels"].to(DEV), c["params"].to(DEV), batch=c["B"], param_grad=True, logit_grad=False)


def test_nan_on_unlabelled_rows():
    c = _case((7, 4, 64, False))
    z = c["logits"].clone()
    z[c["labels"] < 0] = float("nan")
    out, dl, dp, terms = _run(c, logits=z)
    base = _run(c)
    print("NaN on unlabelled rows: loss", float(out[0]), "finite:", bool(torch.isfinite(dl).all()), bool(torch.isfinite(dp).all()))
    for got, want in zip((out, dl, dp, terms), base):
        assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("key", [(7, 5, 65, False), (3, 5, 17, True)], ids=str)
def test_forbidden_transitions_and_large_margins(key):
    """A third of the transitions at -1e4 (the usual 'forbidden' marker), and on every fifth row one class leading by +120 and one
    trailing by -120."""
    C, B, L, packed = key
    c = dict(cases.nll_case(C, B, L, packed, seed=900 + C))
    g = torch.Generator().manual_seed(901 + C)
    p = c["params"].clone()
    tr = p[: C * C].view(C, C)
    forbid = torch.rand(C, C, generator=g) < 0.33
    forbid[torch.arange(C), torch.arange(C)] = False          # staying in a class is always allowed: some path is finite
    tr[forbid] = -1e4
    z = c["logits"].clone()
    rows = torch.arange(0, c["T"], 5)
    z[rows, torch.randint(0, C, (rows.numel(),), generator=g)] += 120.0
    z[rows, torch.randint(0, C, (rows.numel(),), generator=g)] -= 120.0
    c["logits"], c["params"] = z, p
    loss, dz, dp = ref.nll_grads(z, c["labels"], p, c["spans"], normalise=False)
    num, den, _ = ref.nll(z.double(), c["labels"], p, c["spans"])
    c["ref"] = {"loss": float(num) / den, "den": den, "dz": dz, "dp": dp}
    _check(c, f"forbidden / margins {key}")


def test_same_bits_twice_and_anywhere_in_the_batch():
    big = _case((7, 257, 17, False))
    a, b = _run(big), _run(big)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    n = 5 * big["L"]
    small = dict(big, B=5, T=n, logits=big["logits"][:n], labels=big["labels"][:n], spans=big["spans"][:5])
    s = _run(small)
    print("B = 5 alone against the first five of B = 257: dlogits equal", bool(torch.equal(s[1], a[1][:n])),
          "terms equal", bool(torch.equal(s[3], a[3][:n])))
    assert torch.equal(s[1], a[1][:n]) and torch.equal(s[3], a[3][:n])
    # ... and at another position of a wave: the same five dialogues behind two others
    shift = 2 * big["L"]
    moved = dict(big, B=7, T=n + shift, logits=torch.cat([big["logits"][-shift:], big["logits"][:n]]),
                 labels=torch.cat([big["labels"][-shift:], big["labels"][:n]]))
    m = _run(moved)
    assert torch.equal(m[1][shift:], a[1][:n]) and torch.equal(m[3][shift:], a[3][:n])


def _viterbi_reference(logits, mask, params):
    out = []
    for b in range(logits.shape[0]):
        rows = torch.nonzero(~mask[b]).flatten()
        out.append((rows,) + (ref.viterbi(logits[b, rows], params) if rows.numel() else ([], 0.0, torch.zeros(0))))
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["pad", "cu"])
@pytest.mark.parametrize("L", cases.VITERBI_L)
def test_viterbi_against_reference(L, packed):
    logits, mask, params = cases.viterbi_case(L)
    B, _, C = logits.shape
    if packed:
        cu = torch.arange(0, (B + 1) * L, L, dtype=torch.int32).to(DEV)
        pred, score = F.crf_viterbi(logits.reshape(-1, C).to(DEV), mask.reshape(-1).to(DEV), params.to(DEV), cu_seqlens=cu)
    else:
        pred, score = F.crf_viterbi(logits.reshape(-1, C).to(DEV), mask.reshape(-1).to(DEV), params.to(DEV), batch=B)
    pred, score = pred.cpu().view(B, L), score.cpu()
    assert (pred[mask] == -1).all()
    compared = excluded = 0
    for b, (rows, path, best, gaps) in enumerate(_viterbi_reference(logits, mask, params)):
        if rows.numel() == 0:
            assert float(score[b]) == 0.0
            continue
        dev_path = pred[b, rows].long()
        assert ((dev_path >= 0) & (dev_path < C)).all()
        dev_score = float(ref.path_score(logits[b, rows].double(), dev_path, params))
        best = float(best)
        keep = gaps > cases.GAP
        compared += int(keep.sum())
        excluded += int((~keep).sum())
        diff = int((dev_path[keep] != torch.tensor(path)[keep]).sum())
        print(f"viterbi L={L} b={b}: float64 score of the device path {dev_score:.9g}, best {best:.9g}, device's own {float(score[b]):.9g}; "
              f"{diff} labels differ at {int(keep.sum())} compared positions")
        assert abs(dev_score - best) <= 1e-4 * max(1.0, abs(best))
        assert abs(float(score[b]) - best) <= 1e-4 * max(1.0, abs(best))
        assert diff == 0
    share = excluded / max(compared + excluded, 1)
    print(f"viterbi L={L}: {excluded} of {compared + excluded} positions excluded (gap <= {cases.GAP}): {share:.4%}")
    assert share <= cases.MAX_EXCLUDED


def test_viterbi_zero_inputs_give_class_zero():
    B, L, C = 5, 65, 7
    crf = LinearChainCRF(C).to(DEV)
    mask = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    mask[1] = True
    mask[2, 10:20] = True
    path = crf.decode(torch.zeros(B, L, C, device=DEV), mask)
    assert path.dtype == torch.int64 and tuple(path.shape) == (B, L)
    assert (path[mask] == -1).all() and (path[~mask] == 0).all()


@pytest.mark.parametrize("C", [2, 7, 16])
def test_filter_steps_equal_chunk_and_reference(C):
    S, n = 6, 9
    g = torch.Generator().manual_seed(300 + C)
    params = cases.params_block(C, 301 + C)
    logits = torch.randn(S, n, C, generator=g) * 2.0
    n_new = torch.tensor([9, 0, 3, 1, 9, 5], dtype=torch.int32)
    count0 = torch.tensor([0, 4, 0, 2, 7, 0], dtype=torch.int32)
    phi0 = torch.log_softmax(torch.randn(S, C, generator=g), -1)
    # one call of n rows
    phi_chunk = F.crf_filter(logits.to(DEV), params.to(DEV), phi0.clone().to(DEV), count0.to(DEV), n_new=n_new.to(DEV))
    # n calls of one row
    phi_step = phi0.clone().to(DEV)
    count = count0.clone().to(DEV)
    for k in range(n):
        active = (n_new > k).to(DEV)
        F.crf_filter(logits[:, k].contiguous().to(DEV), params.to(DEV), phi_step, count, active=active)
        count += active.int()
    assert torch.equal(phi_step, phi_chunk)
    err = 0.0
    for s in range(S):
        if int(n_new[s]) == 0:
            assert torch.equal(phi_chunk[s].cpu(), phi0[s])
            continue
        want = ref.filter_rows(logits[s, : int(n_new[s])], params, phi0[s].double(), int(count0[s]))[-1]
        err = max(err, float((phi_chunk[s].double().cpu() - want).abs().max()))
    print(f"filter C={C}: max abs err against the float64 filter {err:.3g}")
    assert err <= 1e-5


def test_module_loss_and_gradients():
    """LinearChainCRF.forward: both input layouts, gradients to the logits and to the parameter block; frozen: none to the block."""
    c = _case((7, 4, 64, False))
    B, L, C = 4, 64, 7
    crf = LinearChainCRF(C).to(DEV)
    with torch.no_grad():
        crf.params.copy_(c["params"])
    z = c["logits"].view(B, L, C).to(DEV).requires_grad_(True)
    y = c["labels"].view(B, L).to(DEV)
    loss = crf(z.permute(0, 2, 1), y)
    loss.backward()
    loss2 = crf(z.detach(), y)
    r = c["ref"]
    e_dl = float((z.grad.double().cpu().view(-1, C) * r["den"] - r["dz"]).abs().max())
    e_dp = float((crf.params.grad.double().cpu() * r["den"] - r["dp"]).abs().max()) / float(r["dp"].abs().max())
    print(f"module: loss {float(loss):.9g} ref {r['loss']:.9g}; dlogits err {e_dl:.3g}; dparams err {e_dp:.3g}")
    assert torch.equal(loss, loss2) and abs(float(loss) - r["loss"]) <= 2e-6 * abs(r["loss"])
    assert e_dl <= 1e-5 and e_dp <= 1e-5
    assert crf.transitions.shape == (C, C) and crf.start.shape == (C,) and crf.end.shape == (C,)
    crf.params.requires_grad_(False)
    crf.params.grad = None
    z.grad = None
    crf(z, y).backward()
    assert crf.params.grad is None and z.grad is not None
