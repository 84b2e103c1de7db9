"""The plan compiler's output, pinned (no GPU; needs the built library, as the other dry-plan tests do).  Every case of
tests/golden/make_plan_dumps.py is dry-compiled and its canonical dump -- every command, every descriptor field with pointers
resolved to [region, offset], the arena layouts, lanes, marks, layer maps, output and gradient tensors -- is held to the SHA-256
digests of tests/golden/plan_dumps.json, one per part, so that a failure names the part that moved.  To see WHAT moved, write the
whole dumps of two trees with `make_plan_dumps.py --full DIR` and diff them."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_plan_dumps as D  # noqa: E402

CASES = D.cases()
with open(D.OUT) as _f:
    RECORDED = json.load(_f)


def test_every_case_is_recorded_and_nothing_else():
    assert sorted(RECORDED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_dump_matches_the_recorded_digests(name, monkeypatch, tmp_path):
    case = CASES[name]
    monkeypatch.setenv("DYK_TUNE_CACHE", "0")          # (dry plans never tune; nothing may touch the cache either way)
    for k in D.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    got = D.digests(D.run_case(case, tmp_path))
    want = RECORDED[name]
    assert (got["n_fwd"], got["n_bwd"]) == (want["n_fwd"], want["n_bwd"]), "command counts of %s" % name
    moved = [p for p in D.PARTS if got[p] != want[p]]
    assert not moved, "%s: parts %s differ from the recorded plan" % (name, moved)


def test_deferred_normalise_changes_the_plan_not_its_length():
    """DYK_DW_PRE=1 takes the deferred-normalise path: the same number of commands as the default plan, other descriptors"""
    a, b = RECORDED["cfg3_bf16_train"], RECORDED["c5_train_DYK_DW_PRE=1"]
    assert (a["n_fwd"], a["n_bwd"]) == (b["n_fwd"], b["n_bwd"]) and a["fwd"] != b["fwd"] and a["bwd"] != b["bwd"]
