"""float64 torch reference of the focal criterion (csrc/rowops.hip m2f_ce_focal_kernel; mer_amd.optim.M2FFocalLoss).

Per labelled row t (label y, p = softmax(z_t), class weights w or ones, label smoothing eps, C classes, gamma):

    ce_t  = (1 - eps) * w_y * (-log p_y) + (eps / C) * sum_c w_c * (-log p_c)        (torch's class-weighted, smoothed numerator)
    omp_t = sum_{c != y} p_c                                                        (1 - p_y WITHOUT the subtraction)
    num_t = omp_t^gamma * ce_t                      den_t = w_y
    loss  = sum_t num_t / sum_t den_t

With a teacher (tests/golden/distill_ref.py) the factor scales the hard-label term only:
    num_t = (1 - alpha) * omp_t^gamma * ce_t + alpha * tau^2 * w_y * KL(softmax(u_t / tau) || softmax(z_t / tau)).
gamma = 0 is factor 1 by definition (no 0^0).  Gradients by autograd."""
import torch
import torch.nn.functional as F


def focal_terms(logits, labels, class_w=None, label_smoothing=0.1, gamma=2.0, teacher=None, alpha=0.0, temperature=1.0):
    """-> (num, den) as float64 scalars (num carries the autograd graph of `logits`)."""
    z = logits.double()
    C = z.shape[-1]
    valid = (labels >= 0) & (labels < C)
    w = class_w.double() if class_w is not None else torch.ones(C, dtype=torch.float64, device=z.device)
    zv, yv = z[valid], labels[valid]
    ce_rows = F.cross_entropy(zv, yv, weight=class_w.double() if class_w is not None else None, ignore_index=-1, reduction="none",
                              label_smoothing=label_smoothing)
    p = F.softmax(zv, -1)
    other = torch.ones_like(p).scatter_(1, yv[:, None], 0.0)
    omp = (p * other).sum(-1)                                  # the other classes' probabilities, added
    if gamma == 0:
        factor = torch.ones_like(omp)
    else:
        live = omp > 0                                         # (float64: only at margins beyond ~745)
        factor = torch.where(live, torch.where(live, omp, torch.ones_like(omp)) ** gamma, torch.zeros_like(omp))
    wy = w[yv]
    hard = (factor * ce_rows).sum()
    if teacher is None:
        return hard, wy.sum()
    uv = teacher.detach().double()[valid]
    kl_rows = F.kl_div(F.log_softmax(zv / temperature, -1), F.softmax(uv / temperature, -1), reduction="none").sum(-1)
    return (1.0 - alpha) * hard + alpha * temperature ** 2 * (wy * kl_rows).sum(), wy.sum()


def focal_loss_and_grad(logits, labels, class_w=None, label_smoothing=0.1, gamma=2.0, teacher=None, alpha=0.0, temperature=1.0):
    """-> (loss, den, num, d loss / d logits [T, C]) in float64; the gradient is the NORMALISED one (of num / den)."""
    z = logits.detach().double().clone().requires_grad_(True)
    num, den = focal_terms(z, labels, class_w, label_smoothing, gamma, teacher, alpha, temperature)
    loss = num / den
    loss.backward()
    return loss.detach(), den.detach(), num.detach(), z.grad
