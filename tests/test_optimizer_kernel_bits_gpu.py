"""The optimizer kernels (csrc/adam.hip, csrc/sam.hip; the walks and element functions of csrc/param_walk.h) against the bits recorded in
tests/golden/optimizer_kernel_bits.npz on the commit the fixture names, before the kernels were moved onto the shared walks: every case
of tools/record_optimizer_bits.py, replayed with that file's own case list and input generator, must give every output buffer - p, m, v,
ema, saved, the shadow buffer, pads included - the recorded SHA-256 and the SAM records the recorded floats, bit for bit.  The other
optimizer tests compare the kernels with each other and with float64; this one notices a change that moves them all together."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_optimizer_bits as rec  # noqa: E402

CASES = rec.cases()


@pytest.fixture(scope="module")
def fixture():
    with np.load(rec.FIXTURE) as f:
        return str(f["commit"]), rec.unpack({k: f[k] for k in f.files})


def test_the_fixture_holds_exactly_the_case_list(fixture):
    commit, blocks = fixture
    assert blocks.keys() == {c["id"] for c in CASES} and len(blocks) == len(CASES)
    assert commit and os.path.getsize(rec.FIXTURE) < 64 * 1024
    for c in CASES:
        want = {"adam": {"p", "m", "v"}, "shadowed": {"p", "m", "v", "sh"}, "grouped": {"p", "m", "v"}, "exchange": {"p", "ema"},
                "sam": {"p", "saved", "restored", "record"}}[c["entry"]]
        want = want | ({"ema"} if c.get("ema_w") is not None else set()) | ({"sh"} if c.get("sh") else set())
        assert blocks[c["id"]].keys() == want, c["id"]
        assert all(a.shape == ((rec.STEPS, 4) if k == "record" else (32,)) for k, a in blocks[c["id"]].items())


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_bits_are_the_recorded_ones(case, fixture):
    commit, blocks = fixture
    want = blocks[case["id"]]
    got = rec.run_case(case)
    assert got.keys() == want.keys()
    differ = [k for k in sorted(got) if got[k].dtype != want[k].dtype or got[k].tobytes() != want[k].tobytes()]
    print(f"{case['id']} (recorded on {commit}): {len(got)} buffers, differing: {differ or 'none'}")
    if "record" in got:
        print("  records", got["record"].tolist())
    assert not differ
