"""float64 torch reference of the distillation criterion (csrc/rowops.hip m2f_ce_distill_kernel; mer_amd/distill.py).

Per labelled row t (label y, class weights w or ones, label smoothing eps, temperature tau, alpha):

    num_t = (1 - alpha) * CE_t + alpha * tau^2 * w_y * KL(softmax(u_t / tau) || softmax(z_t / tau))        den_t = w_y
    loss  = sum_t num_t / sum_t den_t

CE_t from ``F.cross_entropy(..., reduction='sum')`` (torch's own class-weighted, label-smoothed numerator), the KL rows from
``F.kl_div(..., reduction='none')``; gradients by autograd."""
import torch
import torch.nn.functional as F


def distill_terms(logits, teacher, labels, class_w=None, label_smoothing=0.1, alpha=0.5, temperature=2.0):
    """-> (num, den) as float64 scalars (num carries the autograd graph of `logits`)."""
    z = logits.double()
    u = teacher.detach().double()
    C = z.shape[-1]
    valid = (labels >= 0) & (labels < C)
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=z.device)
    zv, uv, yv = z[valid], u[valid], labels[valid]
    ce = F.cross_entropy(zv, yv, weight=class_w.double() if class_w is not None else None, ignore_index=-1, reduction="sum",
                         label_smoothing=label_smoothing)
    kl_rows = F.kl_div(F.log_softmax(zv / temperature, -1), F.softmax(uv / temperature, -1), reduction="none").sum(-1)
    wy = w[yv]
    num = (1.0 - alpha) * ce + alpha * temperature ** 2 * (wy * kl_rows).sum()
    return num, wy.sum()


def distill_loss_and_grad(logits, teacher, labels, class_w=None, label_smoothing=0.1, alpha=0.5, temperature=2.0):
    """-> (loss, den, num, d loss / d logits [T, C]) in float64; the gradient is the NORMALISED one (of num / den)."""
    z = logits.detach().double().clone().requires_grad_(True)
    num, den = distill_terms(z, teacher, labels, class_w, label_smoothing, alpha, temperature)
    loss = num / den
    loss.backward()
    return loss.detach(), den.detach(), num.detach(), z.grad


def closed_form_grad(logits, teacher, labels, class_w=None, label_smoothing=0.1, alpha=0.5, temperature=2.0):
    """The UNNORMALISED gradient g[t, c] the kernel writes, from the closed form, in float64:
    (1 - alpha) * gCE + alpha * tau * w_y * (q - p); zero rows where the label is invalid."""
    z, u = logits.detach().double(), teacher.detach().double()
    T, C = z.shape
    valid = (labels >= 0) & (labels < C)
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=z.device)
    y = labels.clamp(0, C - 1)
    wy = w[y]
    p1 = F.softmax(z, -1)
    onehot = F.one_hot(y, C).double()
    eps = label_smoothing
    g_ce = (1.0 - eps) * wy[:, None] * (p1 - onehot) + (eps / C) * (w.sum() * p1 - w[None, :])
    q, p = F.softmax(z / temperature, -1), F.softmax(u / temperature, -1)
    g = (1.0 - alpha) * g_ce + alpha * temperature * wy[:, None] * (q - p)
    return torch.where(valid[:, None], g, torch.zeros_like(g))
