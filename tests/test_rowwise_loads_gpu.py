"""The row-wise kernels issue their independent loads together (LayerNorm forward / backward through range-checked buffer loads,
the attention kernels' pad flags and dropout state with the slabs).  No arithmetic changed with that, so no bit may:

  * every output of the single-kernel entry points - LayerNorm forward / backward (site, residual / extra, masked second output,
    row stride, the general path, two problems in one launch, bf16 shadows), dialogue attention forward / backward (fp32 and the
    bf16 forms, dropout, padded keys), the varlen forms (packed with rows behind the last dialogue, padded), the criterion and the
    row dropout - equals the bits recorded in tests/golden/rowwise_parent_bits.npz from the build in front of the change
    (tests/golden/make_rowwise_parent_bits.py: the cases and the recipe; the test runs the same functions);
  * one bf16 train step of the tiny plan with dropout 0.4 at a fixed rng state gives the recorded logits, loss and flat gradient;
  * on 16-byte-aligned rows the 16-byte path gives what the general path gives (forced by a base pointer 4 bytes off, on a copy of
    the same values), bit for bit.

No tolerance anywhere.  Shapes: T = 5 rows (a partly filled last row block), d = 768 / 1024 / 300 on the 16-byte path (768 under
four chunks per lane leaves a whole chunk out of range, 300 a partly filled one), d = 301 and the offset pointer on the general
path; attention B = 3, H = 2, L in {1, 5, 16}, head dim in {60, 96, 128}.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import make_rowwise_parent_bits as G  # noqa: E402
import mer_amd  # noqa: E402,F401


@pytest.fixture(scope="module")
def recorded():
    with np.load(G.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _same(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    diff = got != want
    n = int(diff.sum())
    print(f"{name}: {got.size} elements, {n} differ from the recorded bits")
    assert n == 0, f"{name}: {n} of {got.size} elements differ (first at {tuple(int(i) for i in np.argwhere(diff)[0])})"


@pytest.mark.parametrize("group", sorted(G.GROUPS))
def test_bits_are_the_recorded_ones(group, recorded):
    got = G.compute(group)
    want = {k: v for k, v in recorded.items() if k.split("/")[0] == group}
    assert sorted(got) == sorted(want) and got, (sorted(got), sorted(want))
    for k in sorted(got):
        _same(k, got[k], want[k])


@pytest.mark.parametrize("d,ld,with_res,site", [(768, 768, True, 4), (1024, 1028, False, 0), (300, 304, True, 4), (2048, 2048, True, 4)])
def test_layernorm_16_byte_path_equals_general_path(d, ld, with_res, site):
    """the same values behind a base pointer that is 4 bytes off a 16-byte boundary take the general path (guarded element loads)"""
    fast = G.ln_run(d, ld, with_res, site, False)
    general = G.ln_run(d, ld, with_res, site, True)
    for k in sorted(fast):
        _same(f"ln d={d} ld={ld} {k}", G.bits(general[k]), G.bits(fast[k]))
