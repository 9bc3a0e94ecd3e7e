"""float64 restatement of the exponential moving average of the weights as the fused optimizer keeps it
(torch.optim.swa_utils.AveragedModel with multi_avg_fn = get_ema_multi_avg_fn(decay), updated once after every optimizer step): the
reference values of tests/test_ema_gpu.py, checked against torch itself in tests/test_ema_cpu.py.

    update n (from 0):   decay_n = decay                                  without warm-up
                         decay_n = min(decay, (1 + n) / (10 + n))         with warm-up
    n == 0:              e = p                                            AveragedModel's n_averaged == 0 copy
    n >= 1:              e = e + (1 - decay_n) * (p - e)                  torch's e.lerp_(p, 1 - decay)

`p` is the exact fp32 parameter after the optimizer step, widened to float64; 1 - decay_n is formed in double.  Everything here is
Python float / float64 tensors; nothing is rounded to fp32.

The bound an fp32 implementation is held to: an update makes at most four roundings - the weight, the subtraction, the product or
fma, the sum - each at most 2^-24 relative to a quantity bounded by 2 M, M the largest magnitude the element's parameter took so far
(the average is a convex combination of those parameters); errors are carried forward with factor decay_n <= 1.  After k updates the
elementwise error is therefore at most 8 k 2^-24 M."""
import torch


def decay_at(decay: float, n: int, warmup: bool = False) -> float:
    """The decay of update `n` (from 0)."""
    decay = float(decay)
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def weight_at(decay: float, n: int, warmup: bool = False) -> float:
    """w = 1 - decay_n in double; update 0 copies (w = 1)."""
    return 1.0 if n == 0 else 1.0 - decay_at(decay, n, warmup)


def update(ema, params: torch.Tensor, decay: float, n: int, warmup: bool = False) -> torch.Tensor:
    """-> the float64 average after update `n` with the parameters `params` (any dtype; widened exactly).  `ema`: the float64 average
    before it (ignored, may be None, for n == 0)."""
    p = params.detach().double()
    if n == 0:
        return p.clone()
    return ema + weight_at(decay, n, warmup) * (p - ema)


def bound(k: int, magnitude: torch.Tensor) -> torch.Tensor:
    """Elementwise error bound of an fp32 average after k updates: 8 k 2^-24 M."""
    return 8.0 * k * 2.0 ** -24 * magnitude.double()


class Average:
    """The float64 average of one buffer over a run, with the running magnitude M = max |p| per element and the update count."""

    def __init__(self, decay: float, warmup: bool = False):
        self.decay, self.warmup = float(decay), bool(warmup)
        self.n = 0
        self.value = None
        self.magnitude = None

    def step(self, params: torch.Tensor, mask=None) -> None:
        """One update from the fp32 parameters read back after an optimizer step.  mask (bool, optional): only those elements are
        averaged; the others keep what they had (zero before the first update)."""
        new = update(self.value, params, self.decay, self.n, self.warmup)
        mag = params.detach().double().abs()
        if mask is not None:
            keep = self.value if self.value is not None else torch.zeros_like(new)
            new = torch.where(mask, new, keep)
            mag = torch.where(mask, mag, torch.zeros_like(mag))
        self.value = new
        self.magnitude = mag if self.magnitude is None else torch.maximum(self.magnitude, mag)
        self.n += 1

    def error_ratio(self, ema: torch.Tensor) -> float:
        """max over the elements of |ema - value| / bound (0 / 0 counts as 0; anything / 0 as inf)."""
        err = (ema.detach().double() - self.value).abs()
        b = bound(self.n, self.magnitude)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
        return float(ratio.max())
