"""Generates tests/golden/dwconv_queries.json: the answers of the two host-side depthwise queries (dyk_dwconv_tile_ok,
dyk_dwconv_wgrad_rows -- neither touches a device or reads a tensor), error codes included, for a table of descriptors, taken
from the library named by DYK_LIB (default: the in-tree build).  dyk_dwconv_tile_ok is the precondition dyk/plan.py relies on for
`pre` and `res`; the plane count of dyk_dwconv_wgrad_rows names the weight-gradient kernel and its grid, hence the summation
order.  tests/test_host_dwconv_queries.py holds the library under test to every row.  The committed table was written by the
library of the commit BEFORE csrc/dwconv.hip got one tile geometry and one route per entry point; regenerate it only when an
answer is meant to change.

Rows (pointers are dummy non-null integers):
  * per (dtype, k 1..7, stride 1..3) a fixed number of seeded draws of channel count, pad 0..3, map and batch
  * every (dtype, k 3 | 5, channel count, batch) at stride 1, pad k // 2 on four maps: the LDS-tiled kernels' domain
  * what check_dw refuses: C % epv (C = 4, 12 in the 16-bit types are in the grid as well), ld % epv, k 0 and 8, zero extents,
    stride 0, an unknown dtype, null x, null y, a null descriptor
C = 32 and 48 stand beside the issue's channel counts: without them no row has channel groups of CT = 4 or 6 vectors.

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_dwconv_queries.py
"""
import ctypes
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "double-yolo-kaist_amd"))

OUT = os.path.join(HERE, "dwconv_queries.json")
COLUMNS = ["dtype", "B", "C", "Hi", "Wi", "Ho", "Wo", "k", "stride", "pad", "ldx", "ldy", "x", "y"]
ANSWERS = ["tile_ok", "wgrad_rows"]
F32, BF16, F16 = 0, 1, 3

CHANNELS = [4, 8, 12, 16, 24, 32, 48, 56, 64, 72, 184, 264, 520, 672, 960, 1024]
KS, STRIDES, PADS = range(1, 8), (1, 2, 3), (0, 1, 2, 3)
MAPS = [(1, 1), (1, 17), (683, 1), (7, 9), (16, 20), (23, 17), (32, 40), (64, 80), (128, 160), (256, 320)]
TILE_MAPS = [(1, 17), (16, 20), (64, 80), (256, 320)]
BATCHES = [1, 3, 32]
N_DRAWS = 40                     # per (dtype, k, stride)
PTR = 4096                       # the queries read no tensor


def epv_of(dtype):
    return 4 if dtype == F32 else 8


def out_size(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def row_of(dt_, b_, c_, h_, w_, k_, s_, pad_, **over):
    ld = -(-c_ // epv_of(dt_)) * epv_of(dt_)
    r = dict(dtype=dt_, B=b_, C=c_, Hi=h_, Wi=w_, Ho=out_size(h_, k_, s_, pad_) if k_ and s_ else h_,
             Wo=out_size(w_, k_, s_, pad_) if k_ and s_ else w_, k=k_, stride=s_, pad=pad_, ldx=ld, ldy=ld, x=PTR, y=PTR)
    r.update(over)
    return r


def make_desc(row):
    """DykDwDesc of a table row (a dict over COLUMNS)"""
    from dyk import lib as L
    d = L.DykDwDesc()
    d.x, d.y = row["x"] or None, row["y"] or None
    for f in ("dtype", "B", "C", "Hi", "Wi", "Ho", "Wo", "k", "stride", "pad", "ldx", "ldy"):
        setattr(d, f, row[f])
    return d


def answers(lib, row):
    d = make_desc(row)
    return [int(lib.dyk_dwconv_tile_ok(ctypes.byref(d))), int(lib.dyk_dwconv_wgrad_rows(ctypes.byref(d)))]


def tile_geometry(row):
    """(CT, tiles, channel groups, workgroups per group) of the LDS-tiled kernels for a 16-bit stride-1 k 3 | 5 row, as
    tests/dwconv_cases.py states the geometry"""
    cv = row["C"] // 8
    groups = (cv + 7) // 8
    ct = -(-cv // groups)
    th = (256 // ct) // 4
    tiles = row["B"] * -(-row["Ho"] // th) * -(-row["Wo"] // 16)
    p0 = min(max(512 // groups, 1), tiles)
    return ct, tiles, groups, -(-tiles // -(-tiles // p0))


def rows():
    rng = random.Random(20250)
    seen = set()
    for dtype, k, s in itertools.product((BF16, F32, F16), KS, STRIDES):
        group = set()
        while len(group) < N_DRAWS:
            C, pad, (H, W), B = rng.choice(CHANNELS), rng.choice(PADS), rng.choice(MAPS), rng.choice(BATCHES)
            if out_size(H, k, s, pad) >= 1 and out_size(W, k, s, pad) >= 1:
                group.add((dtype, B, C, H, W, k, s, pad))
        seen |= group
    for dtype, k, C, B, (H, W) in itertools.product((BF16, F32, F16), (3, 5), CHANNELS, BATCHES, TILE_MAPS):
        seen.add((dtype, B, C, H, W, k, 1, k // 2))
    grid = sorted(seen)
    for col, values in ((0, (BF16, F32, F16)), (1, BATCHES), (2, CHANNELS), (5, KS), (6, STRIDES), (7, PADS)):
        assert {g[col] for g in grid} == set(values), col
    assert {(g[3], g[4]) for g in grid} == set(MAPS)
    out = [row_of(*g) for g in grid]
    # ---- refused descriptors
    base = (BF16, 3, 64, 16, 20, 3, 1, 1)
    out += [row_of(BF16, 3, 12, 16, 20, 3, 1, 1), row_of(F16, 3, 20, 16, 20, 3, 1, 1), row_of(F32, 3, 6, 16, 20, 3, 1, 1),      # C % epv
            row_of(*base, ldx=68), row_of(*base, ldy=68), row_of(F32, 3, 64, 16, 20, 3, 1, 1, ldx=66),                             # ld % epv
            row_of(BF16, 3, 64, 16, 20, 0, 1, 0), row_of(BF16, 3, 64, 16, 20, 8, 1, 4), row_of(F32, 1, 8, 16, 20, 8, 2, 3),        # k 0, 8
            row_of(*base, Hi=0), row_of(*base, Wi=0), row_of(*base, Ho=0), row_of(*base, Wo=0), row_of(*base, B=0), row_of(*base, C=0),
            row_of(BF16, 1, 8, 1, 1, 7, 1, 0),                                                                                     # no output pixel
            row_of(*base, stride=0), row_of(*base, dtype=2), row_of(*base, dtype=4), row_of(*base, dtype=-1),
            row_of(*base, x=0), row_of(*base, y=0),
            row_of(BF16, 3, 12, 16, 20, 0, 1, 0, x=0), row_of(F16, 3, 64, 16, 20, 8, 1, 1, ldx=68)]                                # doubly wrong
    return out


def check_coverage(table, ans):
    """every CT 1..8 at k 3 and k 5 on the tiled forward route, and the persistent weight gradient with more tiles than workgroups"""
    cts, long_walk = set(), 0
    for r, (ok, nrows) in zip(table, ans):
        if ok == 1:
            assert r["dtype"] in (BF16, F16) and r["stride"] == 1 and r["k"] in (3, 5)
            ct, tiles, groups, planes = tile_geometry(r)
            cts.add((r["k"], ct))
            if r["dtype"] == BF16:
                assert nrows == planes, (r, nrows, planes)
                long_walk += nrows < tiles
    assert cts == set(itertools.product((3, 5), range(1, 9))), sorted(cts)
    assert long_walk >= 1
    assert {a[0] for a in ans} >= {1, 0, -1} and {a[1] for a in ans if a[1] < 0} == {-1, -3}
    return long_walk


def main():
    from dyk import lib as L
    lib = L.load()
    table = rows()
    ans = [answers(lib, r) for r in table]
    assert answers(lib, table[0]) == ans[0]
    null = [int(lib.dyk_dwconv_tile_ok(None)), int(lib.dyk_dwconv_wgrad_rows(None))]
    long_walk = check_coverage(table, ans)
    lines = [json.dumps([r[c] for c in COLUMNS] + a, separators=(",", ":")) for r, a in zip(table, ans)]
    with open(OUT, "w") as f:
        f.write('{"library": "%s",\n "columns": %s,\n "null_descriptor": %s,\n "rows": [\n' % (
            lib.dyk_build_sha().decode(), json.dumps(COLUMNS + ANSWERS), json.dumps(null)))
        f.write(",\n".join(lines))
        f.write("\n]}\n")
    print("%s: %d rows (%d tiled weight gradients walk several tiles per workgroup), library %s" % (
        OUT, len(table), long_walk, lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
