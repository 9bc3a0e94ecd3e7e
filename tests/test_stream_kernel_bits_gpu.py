"""The streaming attention kernels (csrc/attention_stream.hip, csrc/attention_stream_chunk.hip) against the bits recorded in
tests/golden/stream_kernel_bits.npz by tools/record_stream_bits.py, on the commit before the dense and the paged kernels became one
body.  The kernels promise the same bits on every run; the other streaming tests hold the paged form to the dense form's bits and
both to float64 inside a tolerance, which a change that moves the two forms together would pass.  Here every case - the case list and
the input generator are the recording tool's - runs in the dense and in the paged form, and each must give the recorded output bytes
and leave caches whose SHA-256 is the recorded one (the pools gathered back through the page table, a non-identity permutation).
A difference is a change in what the kernels compute: the fixture is not recorded again."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mer_amd  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_stream_bits as rec  # noqa: E402

CASES = rec.cases()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return np.load(os.path.join(golden_dir, "stream_kernel_bits.npz"), allow_pickle=False)


def test_the_cases_are_the_ones_recorded(recorded):
    assert sorted(recorded.files) == sorted(c["key"] + "/" + what for c in CASES for what in ("out", "k_sha256", "v_sha256"))
    assert len(CASES) == 20 and {(c["kind"], c["bf16"], c["hd"]) for c in CASES} == {(k, b, h) for k in ("step", "chunk")
                                                                                     for b in (False, True) for h in (20, 128)}


@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
@pytest.mark.parametrize("case", CASES, ids=[c["key"] for c in CASES])
def test_the_bits_are_the_recorded_ones(recorded, case, paged):
    out, ks, vs = rec.run(case, paged)
    want = recorded[case["key"] + "/out"]
    assert out.dtype == want.dtype and out.shape == want.shape
    assert out.tobytes() == want.tobytes(), "the output differs from the recorded bits in %d of %d values" % (
        int((out.view(np.int32) != want.view(np.int32)).sum()), out.size)
    assert ks.tobytes() == recorded[case["key"] + "/k_sha256"].tobytes(), "the K cache after the launch is not the recorded one"
    assert vs.tobytes() == recorded[case["key"] + "/v_sha256"].tobytes(), "the V cache after the launch is not the recorded one"
