"""The depthwise kernels leave the bits recorded in tests/golden/dwconv_bits.json (tests/golden/make_dwconv_bits.py: written on an
MI355X by the commit before csrc/dwconv.hip got one tile geometry, one route per entry point and lost its dead code): the
forward, the data gradient and the weight-gradient planes of every case of tests/dwconv_cases.py in the buffers of
tests/test_gpu_dwconv_elements.py, guard rows and padding channels included; normalise-on-load with six activations; the fused
BatchNorm-backward data gradient; and four single-workgroup launches whose atomics land once per address.  A digest of each
case's inputs is checked first.  Sums that several workgroups add with atomics stay with the fp64 bounds of the element suite."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_dwconv_bits as Q  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "dwconv_bits.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
CASES = Q.cases()


def test_the_fixture_holds_exactly_the_cases_of_the_generator():
    assert sorted(GOLDEN) == sorted(CASES)
    count = lambda s: sum(1 for sec, _ in CASES.values() if sec == s)
    assert count("pre") == 12 and count("res") == 9 and count("single") == 4
    assert count("f") >= 60 and count("d") >= 80 and count("w") >= 40 + len(Q.UNALIGNED)


@pytest.mark.parametrize("cid", list(CASES))
def test_the_launch_leaves_the_recorded_bits(cid):
    want = GOLDEN[cid]
    digest, got = Q.run_case(*CASES[cid])
    assert digest == want["in"], "inputs changed, not the kernel: %s" % cid
    assert got == want["out"], "%s: buffers that differ: %s" % (cid, [k for k in got if got[k] != want["out"].get(k)])
