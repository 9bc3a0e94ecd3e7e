"""torch reference of the supervised contrastive criterion (csrc/supcon.hip; M2FNet.train_step(supcon=), mer_amd.optim.M2FSupConLoss),
written from the formula, float64 by default (`dtype=torch.float32` runs the same statements in plain fp32: the yardstick the kernel
tests measure their bound with).

h_i = row i of the features, y_i its label, w the class weights (or ones), C classes:

    V     = rows with 0 <= y_i < C and ||h_i|| > 0
    z_i   = h_i / ||h_i||,  s_ia = (z_i . z_a) / tau
    A(i)  = V \\ {i},  P(i) = {a in A(i): y_a = y_i},  n_i = |P(i)|
    l_i   = logsumexp_{a in A(i)} s_ia - (1 / n_i) * sum_{p in P(i)} s_ip      for i in V with n_i > 0, else 0
    con   = sum_i w_{y_i} l_i,   den = sum of w_{y_i} over the LABELLED rows (zero-norm rows included),   loss share = lam * con / den

Closed-form gradient of lam * con (unnormalised), c_i = lam * w_{y_i} * [i in V, n_i > 0], p_ia = exp(s_ia - lse_i), m_ia = [y_i = y_a]:

    dz_i = (1 / tau) * sum_{a in A(i)} [c_i (p_ia - m_ia / n_i) + c_a (p_ai - m_ia / n_a)] z_a
    dh_i = (dz_i - (dz_i . z_i) z_i) / ||h_i||                                 zeros outside V

`loop_loss` is the same loss as a plain per-anchor loop for autograd (tests/test_supcon_cpu.py checks the closed form against it)."""
import torch


def supcon(h, y, C, class_w=None, lam=1.0, tau=0.1, dtype=torch.float64):
    """-> dict(rows [N, 4] = (lse, n, l, w l), con, den, grad [N, D] of lam * con w.r.t. h, valid, has), all in `dtype`.  `con` carries
    the autograd graph of `h` when h requires a gradient (the closed form `grad` is computed either way)."""
    h = h.to(dtype)
    N = h.shape[0]
    w = class_w.to(dtype) if class_w is not None else torch.ones(C, dtype=dtype, device=h.device)
    norm = h.norm(dim=1)
    labelled = (y >= 0) & (y < C)
    valid = labelled & (norm > 0)
    wy = w[y.clamp(0, C - 1)]
    z = torch.where(valid[:, None], h / norm.clamp_min(torch.finfo(dtype).tiny)[:, None], torch.zeros_like(h))
    s = (z @ z.T) / tau
    A = valid[:, None] & valid[None, :] & ~torch.eye(N, dtype=torch.bool, device=h.device)
    P = A & (y[:, None] == y[None, :])
    n = P.sum(1).to(dtype)
    anykey = A.any(1)
    # (a row without a key keeps finite entries: logsumexp of an all -inf row would send NaN back through autograd)
    lse = torch.where(anykey, torch.logsumexp(torch.where(anykey[:, None], s.masked_fill(~A, float("-inf")), torch.zeros_like(s)), 1),
                      torch.zeros_like(n))
    has = valid & (n > 0)
    pos = (s * P).sum(1)
    l = torch.where(has, lse - pos / n.clamp_min(1), torch.zeros_like(n))
    rows = torch.stack([lse, torch.where(has, n, torch.zeros_like(n)), l, torch.where(has, wy * l, torch.zeros_like(l))], 1)
    con = rows[:, 3].sum()
    den = (wy * labelled).sum()
    # closed-form gradient
    c = torch.where(has, lam * wy, torch.zeros_like(wy))
    ninv = torch.where(has, 1.0 / n.clamp_min(1), torch.zeros_like(n))
    p = torch.where(A & has[:, None], torch.exp(s - lse[:, None]), torch.zeros_like(s))
    G = c[:, None] * (p - P.to(dtype) * ninv[:, None])
    G = G + G.T
    dz = (G @ z) / tau
    dh = (dz - (dz * z).sum(1, keepdim=True) * z) / norm.clamp_min(torch.finfo(dtype).tiny)[:, None]
    grad = torch.where(valid[:, None], dh, torch.zeros_like(dh))
    return {"rows": rows, "con": con, "den": den, "grad": grad, "valid": valid, "has": has}


def loop_loss(h, y, C, class_w=None, lam=1.0, tau=0.1):
    """lam * con as a plain loop over the anchors in float64, for autograd through `h` (a float64 leaf)."""
    N = h.shape[0]
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=h.device)
    V = [i for i in range(N) if 0 <= int(y[i]) < C and float(h[i].detach().norm()) > 0]
    z = {i: h[i] / h[i].norm() for i in V}
    total = h.sum() * 0
    for i in V:
        A = [a for a in V if a != i]
        Pi = [a for a in A if int(y[a]) == int(y[i])]
        if not Pi:
            continue
        s = torch.stack([(z[i] * z[a]).sum() / tau for a in A])
        sp = torch.stack([(z[i] * z[a]).sum() / tau for a in Pi])
        total = total + lam * w[int(y[i])] * (torch.logsumexp(s, 0) - sp.mean())
    return total


def random_case(N, D, C, seed, device="cpu", ld=None, zeros=0.4):
    """Post-ReLU features with `zeros` of the elements 0 (fp32 [N, D]; ld > D: a view of a [N, ld] buffer), labels in -1 .. C-1, class
    weights; with N >= 8: one all-zero row with a valid label, and class C-1 given to exactly one row."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(N, ld or D, generator=g).abs() * (torch.rand(N, ld or D, generator=g) >= zeros)
    y = torch.randint(-1, C, (N,), generator=g)
    if N >= 8:
        y[y == C - 1] = 0
        y[N // 2] = C - 1                      # a class with a single member
        buf[N // 3] = 0.0                      # an all-zero row ...
        y[N // 3] = 1 % C                      # ... with a valid label
    w = 0.3 + 0.7 * torch.rand(C, generator=g)
    buf = buf.to(device)
    return buf[:, :D], y.to(device), w.to(device)
