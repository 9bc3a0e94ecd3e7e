"""float64 torch reference of the R-Drop criterion (csrc/rowops.hip m2f_ce_rdrop_kernel; mer_amd.optim.M2FRDropLoss).

Every token row r has a twin row t(r) = partner[r] (the same utterance under another dropout mask), or -1.  Per labelled row (label y,
p = softmax(z_r), q = softmax(z_t(r)), class weights w or ones, label smoothing eps, C classes):

    ce_r  = (1 - eps) * w_y * (-log p_y) + (eps / C) * sum_c w_c * (-log p_c)        (torch's class-weighted, smoothed numerator)
    s_r   = 0.5 * (KL(p || q) + KL(q || p))      from the two log-softmaxes; 0 for a row without a twin
    num_r = ce_r + alpha * w_y * s_r             den_r = w_y
    loss  = sum_r num_r / sum_r den_r

The map is an involution over rows of one label, so s_r = s_t(r) and the gradient of the sum with respect to z_r is (closed form)

    dCE_r + alpha * w_y * (p * ((log p - log q) - KL(p || q)) + (p - q)).

Gradients by autograd; `closed_form_grad` is the expression the kernel evaluates."""
import torch
import torch.nn.functional as F


def rdrop_terms(logits, partner, labels, class_w=None, label_smoothing=0.1, alpha=1.0):
    """-> (num, den, kl) as float64 scalars (num and kl carry the autograd graph of `logits`); kl = sum_r w_y * s_r, WITHOUT alpha."""
    z = logits.double()
    T, C = z.shape
    valid = (labels >= 0) & (labels < C)
    has = (partner >= 0) & (partner < T)
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=z.device)
    safe_y = torch.where(valid, labels, torch.zeros_like(labels))
    ce_rows = F.cross_entropy(z, torch.where(valid, labels, torch.full_like(labels, -1)), weight=class_w.double() if class_w is not None else None,
                              ignore_index=-1, reduction="none", label_smoothing=label_smoothing)
    live = valid & has
    rows = live.nonzero().flatten()
    lp = F.log_softmax(z[rows], -1)
    lq = F.log_softmax(z[partner[rows].long()], -1)
    s = 0.5 * ((lp.exp() * (lp - lq)).sum(-1) + (lq.exp() * (lq - lp)).sum(-1))
    wy = w[safe_y]
    kl = (wy[rows] * s).sum()
    num = ce_rows[valid].sum() + alpha * kl
    return num, wy[valid].sum(), kl


def rdrop_loss_and_grad(logits, partner, labels, class_w=None, label_smoothing=0.1, alpha=1.0):
    """-> (loss, den, num, kl, d loss / d logits [T, C]) in float64; the gradient is the NORMALISED one (of num / den)."""
    z = logits.detach().double().clone().requires_grad_(True)
    num, den, kl = rdrop_terms(z, partner, labels, class_w, label_smoothing, alpha)
    loss = num / den
    loss.backward()
    return loss.detach(), den.detach(), num.detach(), kl.detach(), z.grad


def closed_form_grad(logits, partner, labels, class_w=None, label_smoothing=0.1, alpha=1.0):
    """d (sum num) / d logits [T, C] in float64, UNNORMALISED, from the row form the kernel evaluates."""
    z = logits.detach().double()
    T, C = z.shape
    valid = (labels >= 0) & (labels < C)
    has = (partner >= 0) & (partner < T)
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=z.device)
    y = torch.where(valid, labels, torch.zeros_like(labels))
    wy = w[y]
    p = F.softmax(z, -1)
    onehot = F.one_hot(y, C).double()
    eps = label_smoothing
    g = (1.0 - eps) * wy[:, None] * (p - onehot) + (eps / C) * (w.sum() * p - w[None, :])
    tw = torch.where(has, partner.long(), torch.arange(T, device=z.device))
    lp, lq = F.log_softmax(z, -1), F.log_softmax(z[tw], -1)
    q = lq.exp()
    klpq = (p * (lp - lq)).sum(-1, keepdim=True)
    k = p * ((lp - lq) - klpq) + (p - q)
    g = g + alpha * wy[:, None] * k * has[:, None]
    return g * valid[:, None]


def random_pairs(T, C, seed, scale=2.0, unlabelled=0.3, device="cpu"):
    """Rows for the kernel tests: logits [T, C], a twin map that is a RANDOM involution (T odd: one row keeps -1), labels shared by the two
    rows of a pair with about `unlabelled` of the pairs at -1, and class weights."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, C, generator=g) * scale
    perm = torch.randperm(T, generator=g)
    partner = torch.full((T,), -1, dtype=torch.int32)
    a, b = perm[0: T - T % 2: 2], perm[1: T - T % 2: 2]
    partner[a], partner[b] = b.to(torch.int32), a.to(torch.int32)
    y = torch.randint(0, C, (T,), generator=g)
    y[torch.rand(T, generator=g) < unlabelled] = -1
    y[b] = y[a]
    if T % 2:
        y[perm[-1]] = int(perm[-1]) % C                         # the row without a twin is a labelled one
    w = 0.3 + 5.0 * torch.rand(C, generator=g)
    return z.to(device), partner.to(device), y.to(device), w.to(device)
