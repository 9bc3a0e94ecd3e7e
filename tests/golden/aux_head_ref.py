"""torch reference of the auxiliary label head (csrc/aux_head.hip; M2FNet.train_step(aux=), mer_amd.optim.M2FAuxiliaryLoss), written from
the definition, float64 by default (`dtype=torch.float32` runs the same statements in plain fp32: the yardstick the kernel tests measure
their bound with).

h_i = row i of the features, W [A, D] and b [A] the head, s_i the auxiliary label, y_i the emotion label, w the emotion class weights (or
ones), C emotion classes.  A row is LIVE when 0 <= y_i < C and 0 <= s_i < A:

    u_i   = W h_i + b                                                          (every row)
    a_i   = (1 - eps) * -logp_i[s_i] + eps * mean_c -logp_i[c],  logp = log_softmax(u)      (live rows; no class weights of its own)
    term_i = w_{y_i} a_i,   aux = sum_i term_i,   den = sum of w_{y_i} over the rows with an EMOTION label,   loss share = lam * aux / den
    g_ic  = w_{y_i} * (p_ic - (1 - eps) [c = s_i] - eps / A)                   (live rows, else 0)
    dh_i  = lam * sum_c g_ic W[c, :],   dW = lam * g^T h,   db = lam * sum_i g_i           (unnormalised; a dead row's h is never read)
"""
import torch


def aux_head(h, y, s, W, b, C, class_w=None, lam=1.0, eps=0.0, dtype=torch.float64):
    """-> dict(logits [N, A], a [N], rows [N] = w_y a, aux, den, g [N, A], dfeat [N, D], dW [A, D], db [A], live), all in `dtype`."""
    h, W, b = h.to(dtype), W.to(dtype), b.to(dtype)
    A = W.shape[0]
    w = class_w.to(dtype) if class_w is not None else torch.ones(C, dtype=dtype, device=h.device)
    labelled = (y >= 0) & (y < C)
    live = labelled & (s >= 0) & (s < A)
    wy = torch.where(live, w[y.clamp(0, C - 1)], torch.zeros((), dtype=dtype, device=h.device))
    u = h @ W.T + b
    # (a dead row may hold anything - NaN, inf: it is replaced before the softmax, not multiplied away behind it)
    us = torch.where(live[:, None], u, torch.zeros_like(u))
    logp = torch.log_softmax(us, 1)
    onehot = torch.nn.functional.one_hot(s.clamp(0, A - 1), A).to(dtype)
    a = (1.0 - eps) * -(logp * onehot).sum(1) + eps * -logp.mean(1)
    a = torch.where(live, a, torch.zeros_like(a))
    rows = wy * a
    g = wy[:, None] * (logp.exp() - (1.0 - eps) * onehot - eps / A)
    g = torch.where(live[:, None], g, torch.zeros_like(g))
    hs = torch.where(live[:, None], h, torch.zeros_like(h))
    den = (w[y.clamp(0, C - 1)] * labelled).sum()
    return {"logits": u, "a": a, "rows": rows, "aux": rows.sum(), "den": den, "g": g, "dfeat": lam * (g @ W), "dW": lam * (g.T @ hs),
            "db": lam * g.sum(0), "live": live}


def dparams(r):
    """[dW row-major | db] of a result, as the kernels lay the block out."""
    return torch.cat([r["dW"].reshape(-1), r["db"]])


def torch_loss(h, y, s, lin, C, lam=1.0, eps=0.0):
    """lam * aux / den through nn.Linear + F.cross_entropy, float64, for rows that are all live or dead by a -1 in EITHER label and
    without class weights: the definition's own words."""
    u = lin(h)
    dead = (y < 0) | (s < 0)
    ce = torch.nn.functional.cross_entropy(u, torch.where(dead, torch.full_like(s, -1), s), ignore_index=-1, label_smoothing=eps,
                                           reduction="sum")
    return lam * ce / (y >= 0).sum()


def random_case(N, D, A, C, seed, device="cpu", zeros=0.4, margin=None):
    """Post-ReLU features with `zeros` of the elements 0 (fp32 [N, D]), emotion labels in -1 .. C-1, auxiliary labels in -1 .. A (A itself:
    out of range, ignored), the head's block [W | b] and the emotion class weights.  margin: W is scaled so that the logits' spread
    reaches it."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, D, generator=g).abs() * (torch.rand(N, D, generator=g) >= zeros)
    y = torch.randint(-1, C, (N,), generator=g)
    s = torch.randint(-1, A + 1, (N,), generator=g)
    if N >= 8:
        y[0], s[0] = 0, 0                        # at least one live row,
        y[1], s[1] = -1, 1                       # one with an auxiliary label and no emotion label,
        y[2], s[2] = 1 % C, -1                   # and the other way round
    else:
        y[:], s[:] = torch.arange(N) % C, torch.arange(N) % A
    W = torch.randn(A, D, generator=g) / D ** 0.5
    b = 0.1 * torch.randn(A, generator=g)
    if margin is not None:
        u = h @ W.T
        W = W * (margin / (u.max(1).values - u.min(1).values).max().clamp_min(1e-6))
    w = 0.3 + 0.7 * torch.rand(C, generator=g)
    params = torch.cat([W.reshape(-1), b]).contiguous()
    return h.to(device), y.to(device), s.to(device), params.to(device), w.to(device)
