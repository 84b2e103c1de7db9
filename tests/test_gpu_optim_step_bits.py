"""The fused optimizer steps leave the bits recorded in tests/golden/optim_step_bits.json (tests/golden/make_optim_step_bits.py:
written on an MI355X by the commit before the step kernels became one template and the step() bodies of dyk/optim.py one):
every entry point of csrc/optim.hip in one launch on the buffers of tests/test_gpu_optim.py, guard bands included, and the
optimizer classes over three steps on the smallest model.  A digest of each case's inputs is checked first."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_optim_step_bits as Q  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "optim_step_bits.json")) as _f:
    GOLDEN = json.load(_f)
ABI = Q.abi_cases()


def test_the_fixture_holds_exactly_the_cases_of_the_generator():
    assert sorted(GOLDEN["abi"]) == sorted(ABI) and sorted(GOLDEN["objects"]) == sorted(Q.OBJECT_MODES)
    for kind in ("adam", "sgd"):
        for entry in ("plain", "guarded", "groups"):
            assert sum(1 for c in ABI.values() if c["kind"] == kind and c["entry"] == entry) >= 10


@pytest.mark.parametrize("cid", list(ABI))
def test_one_launch_leaves_the_recorded_bits(cid):
    want = GOLDEN["abi"][cid]
    digest, got = Q.run_abi_case(ABI[cid])
    assert digest == want["in"], "inputs changed, not the kernel: %s" % cid
    assert got == want["out"], "%s: buffers that differ: %s" % (cid, [k for k in got if got[k] != want["out"][k]])


@pytest.mark.parametrize("mode", Q.OBJECT_MODES)
def test_the_optimizer_classes_leave_the_recorded_bits(mode):
    want = GOLDEN["objects"][mode]
    digest, got, stats = Q.run_object_mode(mode)
    assert digest == want["in"], "inputs changed, not the kernel: %s" % mode
    assert got == want["out"], "%s: differs in %s" % (mode, [k for k in got if got[k] != want["out"].get(k)])
    assert stats == want["stats"]
    if mode == "adam_guarded":                              # (the inf planted in step 2)
        assert stats == dict(applied_steps=2, skipped_steps=1)
