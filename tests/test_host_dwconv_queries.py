"""The host side of the depthwise convolution -- whether the forward runs a descriptor on the LDS-tiled kernel
(dyk_dwconv_tile_ok: the precondition of `pre` and `res` in dyk/plan.py) and how many planes the weight gradient writes
(dyk_dwconv_wgrad_rows: which kernel, which grid, hence the summation order) -- answers as recorded in
tests/golden/dwconv_queries.json (tests/golden/make_dwconv_queries.py: written by the library before csrc/dwconv.hip got one
tile geometry and one route per entry point), error codes included.  No device is touched."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_dwconv_queries as Q  # noqa: E402


def test_dwconv_queries_answer_as_recorded():
    from dyk import lib as L
    lib = L.load()
    with open(Q.OUT) as f:
        table = json.load(f)
    assert table["columns"] == Q.COLUMNS + Q.ANSWERS
    rows = table["rows"]
    n = len(Q.COLUMNS)
    # the table is the generator's: same descriptors, same order
    assert [r[:n] for r in rows] == [[d[c] for c in Q.COLUMNS] for d in Q.rows()] and len(rows) > 3000
    wrong = []
    for r in rows:
        row, want = dict(zip(Q.COLUMNS, r)), r[n:]
        got = Q.answers(lib, row)
        if got != want:
            wrong.append((row, dict(zip(Q.ANSWERS, want)), dict(zip(Q.ANSWERS, got))))
    assert not wrong, "%d of %d rows differ, first: %s" % (len(wrong), len(rows), wrong[:3])
    assert [int(lib.dyk_dwconv_tile_ok(None)), int(lib.dyk_dwconv_wgrad_rows(None))] == table["null_descriptor"]
    # every channel-group width at both tiled kernel sizes, a persistent weight gradient that walks several tiles per workgroup,
    # and every return code are in the table
    assert Q.check_coverage([dict(zip(Q.COLUMNS, r)) for r in rows], [r[n:] for r in rows]) >= 1
    # an even k: dyk_dwconv_wgrad_rows answers the row kernel's plane count although dyk_dwconv_wgrad refuses the launch
    even = [r for r in rows if r[Q.COLUMNS.index("k")] in (2, 4, 6) and r[Q.COLUMNS.index("dtype")] != Q.F16 and r[n + 1] >= 1]
    assert len(even) > 100
