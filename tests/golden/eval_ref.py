"""Expectations of the device-metrics tests: scikit-learn's own numbers for one batch (the reference's rule, src/train.py:260-272),
seeded label / prediction batches with the corner cases the rule has, and a synthetic collated loader for validate() / test()."""
import warnings

import numpy as np
import torch
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score


def sk_scores(target, predicted):
    """(accuracy, weighted F1) of one batch as the reference's loop computes them; an empty batch gives (nan, nan)."""
    target, predicted = np.asarray(target, dtype=np.int64), np.asarray(predicted, dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(accuracy_score(target, predicted)), float(f1_score(target, predicted, average="weighted"))


def sk_confusion(target, predicted, C):
    target, predicted = np.asarray(target, dtype=np.int64), np.asarray(predicted, dtype=np.int64)
    if target.size == 0:
        return np.zeros((C, C), dtype=np.int64)
    return confusion_matrix(target, predicted, labels=list(range(C))).astype(np.int64)


def label_batches(n, seed=0, C=7, max_rows=1199):
    """n seeded (target, predicted) pairs: 1 .. max_rows rows, 1 .. C classes present, predictions from all-right to all-random."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rows = int(g.integers(1, max_rows + 1))
        present = g.permutation(C)[: int(g.integers(1, C + 1))]
        target = present[g.integers(0, len(present), rows)]
        noise = float(g.choice([0.0, 0.1, 0.5, 1.0]))
        flip = g.random(rows) < noise
        predicted = np.where(flip, g.integers(0, C, rows), target)
        out.append((target.astype(np.int64), predicted.astype(np.int64)))
    return out


CORNERS = {
    "one_class_only": ([3, 3, 3, 3], [3, 3, 3, 3]),
    "one_class_all_wrong": ([2, 2, 2], [5, 5, 1]),
    "only_predicted_classes": ([0, 0, 1, 1], [4, 5, 6, 1]),          # 4, 5, 6 are predicted, never present: weight 0
    "only_present_classes": ([0, 1, 2, 3, 4], [0, 0, 0, 0, 0]),     # 1 .. 4 are present, never predicted: f = 0
    "single_row_right": ([6], [6]),
    "single_row_wrong": ([6], [0]),
    "empty": ([], []),
}


def cm_of(target, predicted, C):
    cm = [[0] * C for _ in range(C)]
    for t, p in zip(target, predicted):
        cm[int(t)][int(p)] += 1
    return cm


def logits_batch(T, C, seed, unlabelled=0.3, ties=False):
    """Seeded logits [T, C] fp32 and labels [T] int64 with about `unlabelled` of the rows at -1 (1.0: every row)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, C, generator=g) * 2.0
    if ties:
        logits = torch.randint(-2, 3, (T, C), generator=g).float()
    labels = torch.randint(0, C, (T,), generator=g)
    if unlabelled >= 1.0:
        labels[:] = -1
    elif unlabelled > 0.0:
        labels[torch.rand(T, generator=g) < unlabelled] = -1
    return logits, labels


def collated_batches(n_batches, d_text, d_audio, C, seed, B=8, max_len=12):
    """A list that stands in for a DataLoader over collate_fn's output: dicts with text / audio / emotion / padding_mask, ragged
    dialogues padded to the batch's longest, the last batch smaller."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n_batches):
        b = B if i < n_batches - 1 else max(B // 2 - 1, 1)
        lens = torch.randint(1, max_len + 1, (b,), generator=g)
        L = int(lens.max())
        mask = torch.arange(L)[None, :] >= lens[:, None]
        emotion = torch.randint(0, C, (b, L), generator=g)
        emotion[mask] = -1
        text = torch.randn(b, L, d_text, generator=g)
        audio = torch.randn(b, L, d_audio, generator=g)
        text[mask] = 0
        audio[mask] = 0
        out.append({"text": text, "audio": audio, "emotion": emotion, "padding_mask": mask})
    return out
