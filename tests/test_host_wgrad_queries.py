"""The host side of the weight gradient -- which kernel a descriptor runs, with how many K splits, and the scratch of the
in-launch fold -- answers as recorded in tests/golden/wgrad_queries.json (tests/golden/make_wgrad_queries.py: written by the
library before the dispatcher and the split planner of csrc/conv_wgrad*.hip were unified).  The split count and the steps per
split decide the summation order, hence the bits of every weight gradient.  No device is touched."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_wgrad_queries as Q  # noqa: E402


def test_wgrad_queries_answer_as_recorded():
    from dyk import lib as L
    lib = L.load()
    with open(Q.OUT) as f:
        table = json.load(f)
    assert table["columns"] == Q.COLUMNS + Q.ANSWERS
    rows = table["rows"]
    with open(os.path.join(Q.ROOT, "bench_tuning.json")) as f:
        n_w = sum(k.startswith("('w'") for k in json.load(f)["choices"])
    assert n_w == 39 and table["bench_rows"] == 2 * n_w and len(rows) > 3000
    # every tune word the plan offers to the tuner and the GPU tests launch is in the table (a new one: regenerate the table)
    assert set(Q.tune_words()) <= {r[Q.COLUMNS.index("tune")] for r in rows}
    wrong = []
    for r in rows:
        row, want = dict(zip(Q.COLUMNS, r)), r[len(Q.COLUMNS):]
        got = Q.answers(lib, row)
        if got != want:
            wrong.append((row, dict(zip(Q.ANSWERS, want)), dict(zip(Q.ANSWERS, got))))
    assert not wrong, "%d of %d rows differ, first: %s" % (len(wrong), len(rows), wrong[:3])
    # every kernel variant, the fold scratch and literal plane counts are in the table
    variants = {r[Q.COLUMNS.index("tune")] >> 28 & 7 for r in rows}, {r[len(Q.COLUMNS) + 1] for r in rows}
    assert variants == ({0, 1, 2, 3}, {0, 1, 2, 3})
    assert any(r[len(Q.COLUMNS) + 2] > 0 for r in rows)
