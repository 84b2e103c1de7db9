"""Generates tests/golden/conv_queries.json: the answers of the two host-side queries of the forward / data-gradient convolution
(dyk_conv_grid, dyk_conv_splitk_ws_bytes -- neither touches a device) for a table of descriptors, and the tuner's candidate
lists (plan._conv_candidates, plan._conv_split_candidates) for the recorded problems, taken from the library named by DYK_LIB
(default: the in-tree build) and the dyk package beside this file.  The queries size the split-K scratch and gate the one-launch
conv + BatchNorm contract; the order of a candidate list decides ties in the tuner: tests/test_host_conv_queries.py holds the
tree under test to every row.  The committed table was written by the commit BEFORE the tune word of the conv front end got
its decoder (csrc/conv_tune.h); regenerate it only when an answer is meant to change.

Rows:
  * the 'c' problems of bench_tuning.json with their recorded tune word and split count (descriptors rebuilt from the key)
  * a seeded sample of  dtype (bf16, f16, f32) x kernel (1x1 | 3x3 / pad 1, stride 1 | 2) x tune word: draws of Cin, Cout, map,
    batch and splitk for every combination.  The words: every candidate of the sampled descriptors, every word
    tests/test_gpu_conv.py launches (candidates with the no-fallback bit, its literals), pointwise words with bit 24 / bit 25,
    large-tile words of shapes 1..3, the K-grouped bit with channel codes 1..3 under every pixel-tile code.  Large-tile words with a patch-width code are drawn without split-K: what the scratch
    query says for them the test asserts by hand (it is where the recorded library launched another tile than it sized).

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_conv_queries.py
"""
import ast
import ctypes
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "double-yolo-kaist_amd"))

OUT = os.path.join(HERE, "conv_queries.json")
COLUMNS = ["dtype", "B", "Cin", "Cout", "Hg", "Wg", "ntaps", "isy", "osy", "flags", "ncls", "tune", "splitk"]
ANSWERS = ["grid", "ws_bytes", "ws_tiles"]
F32, BF16, F16 = 0, 1, 3
NOFALLBACK = 1 << 23

KERNELS = [(1, 1), (1, 2), (3, 1), (3, 2)]                  # (k, stride); pad = k // 2
CHANNELS = [8, 24, 32, 40, 64, 72, 128, 136, 256, 1024]      # (the channel list of make_wgrad_queries.py)
MAPS = [(4, 5), (8, 8), (9, 13), (16, 16), (16, 20), (16, 40), (32, 40), (64, 80), (64, 64)]       # (Hg, Wg): some not divisible by 20 / 8
BATCHES = [1, 2, 3, 16]
SPLITS = [0, 2, 3, 8]


def make_desc(row):
    """DykConvDesc of a table row (a dict over COLUMNS, the fields of plan.autotune's key + tune + splitk); keeps nothing alive:
    the queries read no tensor.  osy == 1: the forward convolution; osy == 2: the data gradient of a stride-2 convolution, all
    four parity classes (ncls == 4) or the class with `ntaps` taps"""
    from dyk import lib as L
    from dyk.ops import dgrad_classes, fwd_taps
    d = L.DykConvDesc()
    epv = 4 if row["dtype"] == F32 else 8
    d.dtype, d.B, d.Cin, d.Cout, d.Hg, d.Wg = (row[c] for c in ("dtype", "B", "Cin", "Cout", "Hg", "Wg"))
    d.ldx, d.ldy = -(-d.Cin // epv) * epv, -(-d.Cout // epv) * epv
    d.isy = d.isx = row["isy"]
    d.osy = d.osx = row["osy"]
    if row["osy"] == 1:
        k = {1: 1, 9: 3}[row["ntaps"]]
        taps = fwd_taps(k, k // 2)
        d.Hi, d.Wi, d.Ho, d.Wo = d.Hg * d.isy, d.Wg * d.isy, d.Hg, d.Wg
    else:
        classes = dgrad_classes(3, 1, row["osy"], d.Hg * row["osy"], d.Wg * row["osy"])
        if row["ncls"] > 1:
            taps, q0 = [t for c in classes for t in c[4]], 0
            for c, (py, px, _, _, ctaps) in enumerate(classes):
                d.cls_first[c], d.cls_ntaps[c], d.cls_ooy[c], d.cls_oox[c] = q0, len(ctaps), py, px
                q0 += len(ctaps)
        else:
            py, px, _, _, taps = next(c for c in classes if len(c[4]) == row["ntaps"])
            d.ooy, d.oox = py, px
        d.Hi, d.Wi, d.Ho, d.Wo = d.Hg, d.Wg, d.Hg * row["osy"], d.Wg * row["osy"]
    assert len(taps) == row["ntaps"]
    d.ntaps = len(taps)
    for q, (ty, tx, wt) in enumerate(taps):
        d.tdy[q], d.tdx[q], d.twt[q] = ty, tx, wt
    d.flags, d.ncls, d.tune, d.splitk = row["flags"], row["ncls"], row["tune"], row["splitk"]
    return d


def answers(lib, row):
    d = make_desc(row)
    nt = ctypes.c_int32(-7)
    ws = int(lib.dyk_conv_splitk_ws_bytes(ctypes.byref(d), ctypes.byref(nt)))
    return [int(lib.dyk_conv_grid(ctypes.byref(d))), ws, nt.value]


def candidates(row):
    """[_conv_candidates(d), _conv_split_candidates(d)] of the row's descriptor, the pairs as lists (JSON)"""
    from dyk import plan as P
    d = make_desc(dict(row, tune=0, splitk=0))
    return [list(P._conv_candidates(d)), [list(c) for c in P._conv_split_candidates(d)]]


def bench_rows():
    with open(os.path.join(ROOT, "bench_tuning.json")) as f:
        choices = json.load(f)["choices"]
    out = []
    for key, (best, _t) in ((ast.literal_eval(k), v) for k, v in choices.items() if k.startswith("('c'")):
        tune, splitk = best if isinstance(best, list) else (best, 0)
        out.append(dict(zip(COLUMNS, list(key[1:]) + [tune, splitk])))
    return out


def sample_pool():
    """the sampled descriptors without a tune word: per (dtype, kernel) seeded draws of the other factors"""
    rng = random.Random(20241)
    pool = []
    for dtype, (k, s) in itertools.product((BF16, F16, F32), KERNELS):
        for _ in range(40):
            (Hg, Wg) = rng.choice(MAPS)
            pool.append(dict(dtype=dtype, B=rng.choice(BATCHES), Cin=rng.choice(CHANNELS), Cout=rng.choice(CHANNELS), Hg=Hg, Wg=Wg,
                             ntaps=k * k, isy=s, osy=1, flags=0, ncls=0))
    return pool


def literal_words():
    """the literal tune words of tests/test_gpu_conv.py, the aliasing cases of csrc/conv_tune.h"""
    words = [0, 64 | (2 << 8) | (1 << 12), 64 | (2 << 8) | (2 << 12), 64 | (2 << 8) | (4 << 12), 128 | (2 << 8) | (2 << 12),
             64 | (3 << 8) | (2 << 24), 64 | (2 << 8) | (2 << 12) | (2 << 24), (6 << 12) | NOFALLBACK, 6 << 12]
    words += [(7 << 12) | (nxs << 8) | (bn << 24) | nf for nxs in (2, 3, 4) for bn in (0, 1, 2) for nf in (0, NOFALLBACK)]
    words += [(5 << 12) | (shape << 8) | (tw << 24) | NOFALLBACK for shape in (1, 2, 3) for tw in (0, 1, 2, 3, 4)]
    words += [(5 << 12) | (shape << 8) for shape in (1, 2, 3)]
    # the K-grouped bit with every channel code under every pixel-tile code (the candidates never pair it with code 1)
    words += [KG_CHAN_WORD(t, bm) for t in range(8) for bm in (1, 2, 3)]
    # the refused-family test: special word, the same with the no-fallback bit, the generic word the route names
    for special, generic in REFUSED_WORDS:
        words += [special, special | NOFALLBACK, generic]
    return words


# (special word, the generic word dyk_conv_route names for it: same K step, stages and channel code) of
# tests/test_gpu_conv.py::test_refused_family_runs_its_generic_tile
REFUSED_WORDS = [
    (64 | (2 << 8) | (3 << 12), 64 | (2 << 8) | (1 << 12)),
    (64 | (2 << 8) | (4 << 12), 64 | (2 << 8) | (2 << 12)),
    (64 | (3 << 8) | (5 << 12), 64 | (3 << 8) | (2 << 12)),
    (64 | (2 << 8) | (7 << 12) | (2 << 24), 64 | (2 << 8) | (0 << 12) | (2 << 24)),
    (64 | (2 << 8) | (2 << 12) | (1 << 28), 64 | (2 << 8) | (2 << 12)),
    (64 | (2 << 8) | (6 << 12), 64 | (2 << 8) | (0 << 12)),
]


def KG_CHAN_WORD(tile, bm):
    return 128 | (2 << 8) | (tile << 12) | (bm << 24) | (1 << 28)


def tune_words(pool=None):
    from dyk import plan as P
    words = literal_words()
    for row in pool if pool is not None else sample_pool():
        d = make_desc(dict(row, tune=0, splitk=0))
        cands = list(P._conv_candidates(d)) + [c for c, _s in P._conv_split_candidates(d)]
        words += cands + [c | NOFALLBACK for c in cands]
    return list(dict.fromkeys(words))


def lt_patch_word(tune):
    return (tune >> 12) & 0xf == 5 and (tune >> 24) & 0xf != 0


def rows():
    out = bench_rows()
    n_bench = len(out)
    pool = sample_pool()
    words = tune_words(pool)
    rng = random.Random(20242)
    seen = set()
    for (k, s), dtype, tune in itertools.product(KERNELS, (BF16, F16, F32), words):
        group = set()
        while len(group) < (1 if dtype == F32 or tune & NOFALLBACK else 2):
            group.add((dtype, rng.choice(BATCHES), rng.choice(CHANNELS), rng.choice(CHANNELS)) + rng.choice(MAPS) +
                      (k * k, s, 1, 0, 0, tune, 0 if lt_patch_word(tune) else rng.choice(SPLITS)))
        seen |= group
    grid = sorted(seen)
    # every value of every factor meets every kernel size
    kernel = lambda g: (g[6], g[7])
    for values, of in (((BF16, F16, F32), lambda g: g[0]), (BATCHES, lambda g: g[1]), (CHANNELS, lambda g: g[2]),
                       (CHANNELS, lambda g: g[3]), (MAPS, lambda g: (g[4], g[5])), (words, lambda g: g[11]), (SPLITS, lambda g: g[12])):
        assert {(kernel(g), of(g)) for g in grid} == set(itertools.product([(k * k, s) for k, s in KERNELS], values))
    assert not any(lt_patch_word(g[11]) and g[12] > 1 for g in grid)
    return out + [dict(zip(COLUMNS, g)) for g in grid], n_bench


def main():
    from dyk import lib as L
    lib = L.load()
    table, n_bench = rows()
    lines = [json.dumps([r[c] for c in COLUMNS] + answers(lib, r), separators=(",", ":")) for r in table]
    cands = [json.dumps(candidates(r), separators=(",", ":")) for r in table[:n_bench]]
    with open(OUT, "w") as f:
        f.write('{"library": "%s",\n "columns": %s,\n "bench_rows": %d,\n "rows": [\n' % (
            lib.dyk_build_sha().decode(), json.dumps(COLUMNS + ANSWERS), n_bench))
        f.write(",\n".join(lines))
        f.write('\n],\n "bench_candidates": [\n')
        f.write(",\n".join(cands))
        f.write("\n]}\n")
    print("%s: %d rows (%d of bench_tuning.json), library %s" % (OUT, len(table), n_bench, lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
