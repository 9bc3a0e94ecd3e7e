"""Restatement in torch on the CPU of the model watch's per-tensor rules (csrc/tensor_stats.hip, mer_amd.watch): the fields in float64,
the histogram by torch.histc's rule spelled out in IEEE fp32 - pos = (int)((x - lo) * bins / (hi - lo)), one subtraction, one
multiplication by the bin count as a float, one division, in that order; pos == bins counted in the last bin; lo, hi = the finite min
and max, lo - 1 and hi + 1 when they are equal.  The GPU tests take their reference values from here; tests/test_watch_cpu.py holds
this file to torch.histc count for count."""
import math

import torch


def histogram(x: torch.Tensor, bins: int, lo: float, hi: float) -> torch.Tensor:
    """int64 [bins] counts of the FINITE fp32 values `x` by the fp32 rule above; lo, hi are fp32 values."""
    x = x.reshape(-1).float()
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    if lo32 == hi32:
        lo32, hi32 = lo32 - 1.0, hi32 + 1.0
    pos = ((x - lo32) * torch.tensor(float(bins), dtype=torch.float32) / (hi32 - lo32)).to(torch.int64)
    return torch.bincount(pos.clamp_(0, bins - 1), minlength=bins)


def tensor_stats(x: torch.Tensor, bins: int) -> dict:
    """`x`: one tensor's values as fp32 (bf16 values widened; for the difference form a - b computed in fp32).  -> numel, finite, nan,
    inf, zeros, min, max (floats; NaN without a finite value), sum, sumsq (float64 sums of the finite values), abs_sum (for the bound on
    sum), mean, l2, rms, hist (int64 [bins]), lo, hi (the histogram's range)."""
    x = x.detach().reshape(-1).float().cpu()
    fin = torch.isfinite(x)
    f = x[fin]
    out = {"numel": x.numel(), "finite": int(fin.sum()), "nan": int(torch.isnan(x).sum()), "inf": int(torch.isinf(x).sum()),
           "zeros": int((x == 0).sum())}
    if f.numel() == 0:
        nan = float("nan")
        out.update(min=nan, max=nan, sum=nan, sumsq=nan, abs_sum=nan, mean=nan, l2=nan, rms=nan, lo=nan, hi=nan,
                   hist=torch.zeros(bins, dtype=torch.int64))
        return out
    d = f.double()
    lo, hi = float(f.min()), float(f.max())
    s, q = float(d.sum()), float((d * d).sum())
    out.update(min=lo, max=hi, sum=s, sumsq=q, abs_sum=float(d.abs().sum()), mean=s / f.numel(), l2=math.sqrt(q),
               rms=math.sqrt(q / f.numel()), hist=histogram(f, bins, lo, hi))
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    if lo32 == hi32:
        lo32, hi32 = lo32 - 1.0, hi32 + 1.0
    out.update(lo=float(lo32), hi=float(hi32))
    return out


def buffer_stats(buf: torch.Tensor, items, bins: int, other: torch.Tensor = None):
    """Per tensor of a flat buffer: `items` = [(offset, numel)] in parameter-map order; `other`: the fp32 difference buf - other."""
    buf = buf.detach().cpu()
    if other is not None:
        buf = buf.float() - other.detach().cpu().float()             # one fp32 subtraction per element
    return [tensor_stats(buf[o: o + n], bins) for o, n in items]
