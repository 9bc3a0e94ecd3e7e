"""float64 reference of the linear-chain CRF (csrc/crf.hip; mer_amd.crf.LinearChainCRF).

For one dialogue with chain emissions e [n, C] (the rows of the chain only, in order), labels y [n] and the parameter block
[transitions C x C | start C | end C]:

    score(y) = start[y_1] + sum_k e[k, y_k] + sum_{k>=2} transitions[y_{k-1}, y_k] + end[y_n]
    logZ     = log sum_paths exp(score)                 (the plain log-space alpha recursion, under autograd)
    loss     = sum_dialogues (logZ - score(y)) / sum_dialogues n

and, independent of the recursion, brute-force enumeration of all C^n paths (logZ, marginals, pair marginals, best path), Viterbi
with max-marginals, and the forward filter.  Everything is torch float64 on the CPU."""
import itertools

import torch

NEG = float("-inf")


def split(params, C):
    params = params.double()
    return params[: C * C].view(C, C), params[C * C: C * C + C], params[C * C + C:]


def log_z(e, params):
    """logZ of one chain, e [n, C] float64 (n >= 1): the plain log-alpha recursion."""
    C = e.shape[1]
    trans, start, end = split(params, C)
    alpha = start + e[0]
    for k in range(1, e.shape[0]):
        alpha = e[k] + torch.logsumexp(alpha[:, None] + trans, 0)
    return torch.logsumexp(alpha + end, 0)


def path_score(e, y, params):
    C = e.shape[1]
    trans, start, end = split(params, C)
    n = e.shape[0]
    s = start[y[0]] + e[torch.arange(n), y].sum() + end[y[-1]]
    if n > 1:
        s = s + trans[y[:-1], y[1:]].sum()
    return s


def chains(labels, spans):
    """The chain rows of every dialogue: spans = [(r0, r1), ...] over the token rows, labels int64 [T] -> list of row-index tensors."""
    out = []
    for r0, r1 in spans:
        rows = torch.arange(r0, r1)
        out.append(rows[labels[r0:r1] >= 0])
    return out


def nll(logits, labels, params, spans):
    """-> (num, den): float64 scalars, num with the autograd graph of `logits` / `params`; per-dialogue nums as a list too."""
    z = logits.double()
    labels = labels.cpu()
    nums, den = [], 0
    for rows in chains(labels, spans):
        if rows.numel() == 0:
            continue
        e, y = z[rows], labels[rows]
        nums.append(log_z(e, params) - path_score(e, y, params))
        den += rows.numel()
    num = torch.stack(nums).sum() if nums else z.sum() * 0.0
    return num, den, nums


def nll_grads(logits, labels, params, spans, normalise=True):
    """-> loss, dlogits [T, C], dparams, all float64 (the gradients of num, divided by den when `normalise`)."""
    z = logits.detach().double().cpu().requires_grad_(True)
    p = params.detach().double().cpu().requires_grad_(True)
    # unlabelled rows never enter the graph: NaN there must not matter
    num, den, _ = nll(z, labels, p, spans)
    if den == 0:
        return num.detach(), torch.zeros_like(z), torch.zeros_like(p)
    dz, dp = torch.autograd.grad(num, (z, p), allow_unused=True)
    dz = torch.zeros_like(z) if dz is None else dz
    dp = torch.zeros_like(p) if dp is None else dp
    scale = 1.0 / den if normalise else 1.0
    return (num / den).detach(), dz * scale, dp * scale


def enumerate_paths(e, params):
    """Brute force over all C^n paths of one chain -> dict(logZ, marginals [n, C], pairs [n-1, C, C], best (list), best_score)."""
    e = e.double()
    n, C = e.shape
    paths = torch.tensor(list(itertools.product(range(C), repeat=n)), dtype=torch.long)          # lexicographic: first max = lowest
    scores = torch.stack([path_score(e, p, params) for p in paths])
    logZ = torch.logsumexp(scores, 0)
    w = torch.exp(scores - logZ)
    marg = torch.zeros(n, C, dtype=torch.float64)
    for k in range(n):
        marg[k].index_add_(0, paths[:, k], w)
    pairs = torch.zeros(max(n - 1, 0), C, C, dtype=torch.float64)
    for k in range(n - 1):
        pairs[k].view(-1).index_add_(0, paths[:, k] * C + paths[:, k + 1], w)
    b = int(torch.argmax(scores))
    return {"logZ": logZ, "marginals": marg, "pairs": pairs, "best": paths[b].tolist(), "best_score": scores[b]}


def marginals(e, params):
    """Marginals [n, C] and pair marginals [n-1, C, C] of one chain by the log-space forward-backward recursion."""
    e = e.double()
    n, C = e.shape
    trans, start, end = split(params, C)
    alpha = [start + e[0]]
    for k in range(1, n):
        alpha.append(e[k] + torch.logsumexp(alpha[-1][:, None] + trans, 0))
    beta = [end]
    for k in range(n - 1, 0, -1):
        beta.append(torch.logsumexp(trans + (e[k] + beta[-1])[None, :], 1))
    beta = beta[::-1]
    logZ = torch.logsumexp(alpha[-1] + end, 0)
    marg = torch.stack([torch.exp(alpha[k] + beta[k] - logZ) for k in range(n)])
    pairs = [torch.exp(alpha[k][:, None] + trans + (e[k + 1] + beta[k + 1])[None, :] - logZ) for k in range(n - 1)]
    return marg, (torch.stack(pairs) if pairs else torch.zeros(0, C, C, dtype=torch.float64)), logZ


def viterbi(e, params):
    """-> (path list, score, gaps [n]): the best path under the first-max rule, its score, and per position the max-marginal gap - the
    best score of ANY path through the position's best class minus the best through its runner-up class (a small gap: the label at
    that position is decided by rounding)."""
    e = e.double()
    n, C = e.shape
    trans, start, end = split(params, C)
    delta = [start + e[0]]
    back = []
    for k in range(1, n):
        cand = delta[-1][:, None] + trans
        back.append(torch.argmax(cand, 0))               # torch.argmax on a CPU float64 tensor returns the first maximum
        delta.append(e[k] + cand.max(0).values)
    final = delta[-1] + end
    cur = int(torch.argmax(final))
    score = final[cur]
    path = [cur]
    for k in range(n - 2, -1, -1):
        cur = int(back[k][cur])
        path.append(cur)
    path = path[::-1]
    bwd = [end]
    for k in range(n - 1, 0, -1):
        bwd.append((trans + (e[k] + bwd[-1])[None, :]).max(1).values)
    bwd = bwd[::-1]
    gaps = []
    for k in range(n):
        mm = torch.sort(delta[k] + bwd[k], descending=True).values
        gaps.append(float(mm[0] - mm[1]))
    return path, score, torch.tensor(gaps, dtype=torch.float64)


def filter_rows(e, params, phi=None, count=0):
    """The forward filter over the rows e [n, C] of one slot, from state (phi, count) -> phi after every row [n, C]."""
    e = e.double()
    C = e.shape[1]
    trans, start, _ = split(params, C)
    out = []
    for k in range(e.shape[0]):
        a = start + e[k] if count + k == 0 else e[k] + torch.logsumexp(phi[:, None] + trans, 0)
        phi = a - torch.logsumexp(a, 0)
        out.append(phi)
    return torch.stack(out)
