"""The BatchNorm/activation kernels of csrc/bn_act.hip and the squeeze-excitation and max-pool kernels of csrc/elementwise.hip leave the
bits recorded in tests/golden/bn_act_bits.json (tests/golden/make_bn_act_bits.py: written on an MI355X by the commit before these
kernels moved onto the shared pieces of csrc/ew_strip.h): every launch of the generator's case groups in the sentinel-framed buffers
of the two element suites, guard rows, padding channels and frames included.  The reduce launches run with one replica per workgroup,
so that every address receives one atomic onto zero; sums that several workgroups add onto one address stay with the fp64 bounds of
the element suites.  A digest of each case's inputs is checked first."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_bn_act_bits as Q  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "bn_act_bits.json")) as _f:
    GOLDEN = json.load(_f)["cases"]
CASES = Q.cases()


def test_the_fixture_holds_exactly_the_cases_of_the_generator():
    assert sorted(GOLDEN) == sorted(CASES)
    count = lambda s: sum(1 for c in CASES if c.startswith(s + "-") or c == s)
    assert (count("fin"), count("fold"), count("params"), count("big"), count("twin")) == (4, 1, 3, 3, 1)
    assert count("fwd") == 12 and count("fused") == count("apply") == count("reduce") == 9
    assert count("se_pool") == 4 and count("se_scale") == 5 and count("pool") == 10
    launches = lambda s: sum(len(v["out"]) for c, v in GOLDEN.items() if c.startswith(s + "-"))
    assert launches("fwd") == 12 * 28 and launches("fused") == 9 * 49 and launches("apply") == 9 * 85 and launches("reduce") == 9 * 7


@pytest.mark.parametrize("cid", list(CASES))
def test_the_launches_leave_the_recorded_bits(cid):
    want = GOLDEN[cid]
    digest, got = Q.run_case(*CASES[cid])
    assert digest == want["in"], "inputs changed, not the kernel: %s" % cid
    assert got == want["out"], "%s: launches that differ: %s" % (cid, [k for k in got if got[k] != want["out"].get(k)])
