"""The host side of the forward / data-gradient convolution -- the grid and the split-K scratch a descriptor's tune word asks
for, the tuner's candidate lists, and the route of dyk_conv_igemm (kernel family + generic fallback) -- answers as recorded in
tests/golden/conv_queries.json (tests/golden/make_conv_queries.py: written by the commit before the tune word got its decoder,
csrc/conv_tune.h) and as the hand-written truth table below, which was read off the if-ladder that commit routed with.
No device is touched."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_conv_queries as Q  # noqa: E402

TUNE = Q.COLUMNS.index("tune")


def _table():
    with open(Q.OUT) as f:
        return json.load(f)


def test_conv_queries_answer_as_recorded():
    from dyk import lib as L
    lib = L.load()
    table = _table()
    assert table["columns"] == Q.COLUMNS + Q.ANSWERS
    rows = table["rows"]
    with open(os.path.join(Q.ROOT, "bench_tuning.json")) as f:
        n_c = sum(k.startswith("('c'") for k in json.load(f)["choices"])
    assert n_c == 123 and table["bench_rows"] == n_c and len(rows) > 3000
    assert [r[:len(Q.COLUMNS)] for r in rows[:n_c]] == [[b[c] for c in Q.COLUMNS] for b in Q.bench_rows()]
    # every tune word the plan offers to the tuner for the sampled descriptors and the GPU tests launch is in the table (a new
    # one: regenerate the table), with the aliasing cases of csrc/conv_tune.h
    words = {r[TUNE] for r in rows}
    assert set(Q.tune_words()) <= words
    assert {(7 << 12) | (2 << 8) | (1 << 24), (7 << 12) | (2 << 8) | (1 << 25)} <= words
    assert {(5 << 12) | (shape << 8) for shape in (1, 2, 3)} <= words
    # the K-grouped bit with channel code 1 on more than 64 channels under split-K: the scratch is sized for 64 rows there
    C = Q.COLUMNS.index
    assert {(r[TUNE] >> 12) & 0xf for r in rows if r[TUNE] >> 28 == 1 and (r[TUNE] >> 24) & 0xf == 1 and r[C("Cout")] > 64
            and r[C("splitk")] > 1} >= {0, 1, 2, 3, 4, 6, 7}
    assert {r[Q.COLUMNS.index("splitk")] for r in rows} >= set(Q.SPLITS) and {r[0] for r in rows} == {Q.F32, Q.BF16, Q.F16}
    wrong = []
    for r in rows:
        row, want = dict(zip(Q.COLUMNS, r)), r[len(Q.COLUMNS):]
        assert not (Q.lt_patch_word(row["tune"]) and row["splitk"] > 1)        # (asserted by hand below)
        got = Q.answers(lib, row)
        if got != want:
            wrong.append((row, dict(zip(Q.ANSWERS, want)), dict(zip(Q.ANSWERS, got))))
    assert not wrong, "%d of %d rows differ, first: %s" % (len(wrong), len(rows), wrong[:3])
    assert any(r[len(Q.COLUMNS) + 1] > 0 for r in rows)


def test_large_tile_fallback_ignores_the_patch_code():
    """pixel-tile code 5 keeps a patch-width code in bits 24..27: its generic 160-pixel fallback takes the channel tile by Cout
    (the recorded library sized the scratch this way too, but launched with the patch code read as a channel tile: the one
    launch that changed with csrc/conv_tune.h).  Scratch = S * 4 bytes * tiles * tile area, the larger of the fallback and the large tile itself."""
    from dyk import lib as L
    lib = L.load()
    # 128 channels, 2 x 16 x 20 = 640 pixels, S = 2; patch code 1 would read as "32 rows" -- the fallback is 128 x 160: 1 x 4 tiles;
    # the 128 x 320 large tile: 1 x 2 tiles of twice the area -- the same bytes
    row = dict(dtype=Q.BF16, B=2, Cin=64, Cout=128, Hg=16, Wg=20, ntaps=9, isy=1, osy=1, flags=0, ncls=0,
               tune=(5 << 12) | (1 << 8) | (1 << 24), splitk=2)
    assert Q.answers(lib, row)[1:] == [2 * 4 * 4 * 128 * 160, 4]
    # 40 channels, 9 x 13 = 117 pixels, S = 3; patch code 3 would read as "128 rows" -- the fallback is 64 x 160: one tile; the
    # 128 x 160 two-group large tile: one tile of twice the area
    row = dict(dtype=Q.BF16, B=1, Cin=64, Cout=40, Hg=9, Wg=13, ntaps=9, isy=1, osy=1, flags=0, ncls=0,
               tune=(5 << 12) | (3 << 8) | (3 << 24), splitk=3)
    assert Q.answers(lib, row)[1:] == [3 * 4 * 1 * 128 * 160, 1]
    # the grid query (the tile DYK_EPI_BNFWD runs, which never runs the large-tile family) reads the word as the recorded library
    # did: 128-pixel tile, bits 24..27 as a channel code -- 32 rows: 4 x 5 tiles
    row = dict(row, Cout=128, tune=(5 << 12) | (1 << 8) | (1 << 24), B=5)
    assert Q.answers(lib, row)[0] == 4 * 5


def test_kgrouped_scratch_is_sized_for_at_least_64_rows():
    """under the K-grouped bit the scratch query reads the channel code and lifts 32 rows to 64, whichever kernel takes the
    problem (as the recorded library did): 136 channels, 117 pixels, S = 2, 128-pixel tile, channel code 1 -> 3 x 1 tiles of 64 x 128"""
    from dyk import lib as L
    row = dict(dtype=Q.BF16, B=1, Cin=128, Cout=136, Hg=9, Wg=13, ntaps=1, isy=1, osy=1, flags=0, ncls=0,
               tune=Q.KG_CHAN_WORD(0, 1), splitk=2)
    assert Q.answers(L.load(), row)[1:] == [2 * 4 * 3 * 64 * 128, 3]
    assert Q.answers(L.load(), dict(row, Cout=72))[1:] == [2 * 4 * 2 * 64 * 128, 2]
    assert Q.answers(L.load(), dict(row, tune=Q.KG_CHAN_WORD(2, 1)))[1:] == [2 * 4 * 3 * 64 * 160, 3]


def test_conv_candidate_lists_are_unchanged():
    """element for element and in order (the order decides ties in the tuner)"""
    table = _table()
    rows, recorded = table["rows"][:table["bench_rows"]], table["bench_candidates"]
    assert len(recorded) == len(rows) == 123
    n_single = n_split = 0
    for r, want in zip(rows, recorded):
        got = Q.candidates(dict(zip(Q.COLUMNS, r)))
        assert got == want, (r, want, got)
        n_single, n_split = n_single + len(got[0]), n_split + len(got[1])
    assert n_single > 1000 and n_split > 100


# ---- route truth table.  Read off the ladder of the commit before csrc/conv_tune.h: DYK_EPI_BNFWD -> generic tiles only
# (codes 1, 3 -> 80 pixels, 2, 4 -> 160, the rest 128); else code 5 -> large-tile | 160; 6 -> resident-weight | 128 (bf16 without
# split-K, else straight to 128); 7 -> pointwise | 128; then the K-grouped bit -> K-grouped, which builds codes 1 and 2 only and
# otherwise hands on to what the code means; then codes 3 / 4 -> halo | 80 / 160; then 1 -> 80, 2 -> 160, the rest 128.  fp32:
# every code reads as 0.  `|` = the generic tile after DYK_ERR_UNSUPPORTED; bit 23 forbids it.
N128, N80, N160, HALO4, HALO8, LT, SC, PW, KGF = range(9)
KG, BNFWD, STATS, NOFB = 1 << 28, 128, 4, 1 << 23
ROUTES = [
    # (dtype, tune, flags, splitk) -> (family, fallback tile)
    ((Q.BF16, 0 << 12, 0, 0), (N128, -1)),
    ((Q.BF16, 1 << 12, 0, 0), (N80, -1)),
    ((Q.BF16, 2 << 12, 0, 0), (N160, -1)),
    ((Q.BF16, 3 << 12, 0, 0), (HALO4, N80)),
    ((Q.BF16, 4 << 12, 0, 0), (HALO8, N160)),
    ((Q.BF16, 5 << 12 | 1 << 8, 0, 0), (LT, N160)),
    ((Q.BF16, 6 << 12, 0, 0), (SC, N128)),
    ((Q.BF16, 7 << 12 | 1 << 24, 0, 0), (PW, N128)),
    ((Q.F16, 4 << 12, 0, 0), (HALO8, N160)),
] + [((Q.F32, t << 12, 0, 0), (N128, -1)) for t in range(8)] + [
    ((Q.F32, 2 << 12 | KG, 0, 0), (N128, -1)),
    ((Q.BF16, 1 << 12, BNFWD | STATS, 0), (N80, -1)),
    ((Q.BF16, 2 << 12, BNFWD | STATS, 0), (N160, -1)),
    ((Q.BF16, 3 << 12, BNFWD | STATS, 0), (N80, -1)),
    ((Q.BF16, 4 << 12, BNFWD | STATS, 0), (N160, -1)),
    ((Q.BF16, 5 << 12 | 1 << 8, BNFWD | STATS, 0), (N128, -1)),
    ((Q.BF16, 6 << 12, BNFWD | STATS, 0), (N128, -1)),
    ((Q.BF16, 7 << 12, BNFWD | STATS, 0), (N128, -1)),
    ((Q.BF16, 2 << 12 | KG, BNFWD | STATS, 0), (N160, -1)),
    ((Q.BF16, 0 << 12 | KG, 0, 0), (N128, -1)),
    ((Q.BF16, 1 << 12 | KG, 0, 0), (KGF, N80)),
    ((Q.BF16, 2 << 12 | KG, 0, 2), (KGF, N160)),
    ((Q.F16, 2 << 12 | KG, 0, 0), (KGF, N160)),
    ((Q.BF16, 3 << 12 | KG, 0, 0), (HALO4, N80)),
    ((Q.BF16, 4 << 12 | KG, 0, 0), (HALO8, N160)),
    ((Q.BF16, 5 << 12 | 3 << 8 | KG, 0, 0), (LT, N160)),
    # the K-grouped family was tried first and refuses every code it does not build: with bit 23 nothing runs
    ((Q.BF16, 0 << 12 | KG | NOFB, 0, 0), (-3, -1)),
    ((Q.BF16, 3 << 12 | KG | NOFB, 0, 0), (-3, -1)),
    ((Q.BF16, 2 << 12 | KG | NOFB, 0, 0), (KGF, N160)),
    # code 6 routes to its family whatever splitk / dtype say: the launch refuses them (bit 23: DYK_ERR_UNSUPPORTED) -> 128
    ((Q.BF16, 6 << 12, 0, 2), (SC, N128)),
    ((Q.F16, 6 << 12, 0, 0), (SC, N128)),
    ((Q.BF16, 9 << 12, 0, 0), (N128, -1)),
]


def test_conv_route_truth_table():
    from dyk import lib as L
    lib = L.load()
    assert L.EPI_BNFWD == BNFWD and L.EPI_STATS == STATS and (L.DYK_F32, L.DYK_BF16, L.DYK_F16) == (Q.F32, Q.BF16, Q.F16)
    assert lib.dyk_conv_route(None, None) == -1
    for (dtype, tune, flags, splitk), want in ROUTES:
        d = Q.make_desc(dict(dtype=dtype, B=1, Cin=64, Cout=64, Hg=16, Wg=20, ntaps=9, isy=1, osy=1, flags=flags, ncls=0,
                             tune=tune, splitk=splitk))
        fb = ctypes.c_int32(-7)
        got = (lib.dyk_conv_route(ctypes.byref(d), ctypes.byref(fb)), fb.value)
        assert got == want, (dtype, hex(tune), flags, splitk, got, want)
        assert lib.dyk_conv_route(ctypes.byref(d), None) == want[0]
