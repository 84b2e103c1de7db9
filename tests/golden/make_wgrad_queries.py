"""Generates tests/golden/wgrad_queries.json: the answers of the three host-side weight-gradient queries
(dyk_conv_wgrad_splits, dyk_conv_wgrad_variant, dyk_conv_wgrad_fold_ws_bytes -- none of them touches a device) for a table of
descriptors, taken from the library named by DYK_LIB (default: the in-tree build).  The split count and the kernel variant
decide the summation order of a weight gradient, hence the bits of the result: tests/test_host_wgrad_queries.py holds the
library under test to every row.  The committed table was written by the library of the commit BEFORE the dispatcher / split
planner of csrc/conv_wgrad*.hip were unified; regenerate it only when an answer is meant to change.

Rows:
  * the 'w' problems of bench_tuning.json with their recorded tune word and split count (descriptors as plan.autotune's)
  * a sample of the grid  kernel (1x1 stride 1 | 2, 3x3 / pad 1 stride 1 | 2) x dtype x Cin x Cout x map x batch x tune word
    x splits x plane mode: every (kernel, dtype, tune word) with a fixed number of seeded draws of the rest; the script checks
    that every value of every factor meets every kernel size

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_wgrad_queries.py
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

OUT = os.path.join(HERE, "wgrad_queries.json")
COLUMNS = ["dtype", "B", "Cin", "Cout", "Ho", "Wo", "k", "stride", "tune", "splits", "part"]
ANSWERS = ["n_splits", "variant", "fold_bytes", "fold_tiles"]
BF16, F32 = 1, 0

KERNELS = [(1, 1), (1, 2), (3, 1), (3, 2)]                  # (k, stride); pad = k // 2
CHANNELS = [8, 24, 32, 40, 64, 72, 128, 136, 256, 1024]
MAPS = [(4, 5), (8, 8), (9, 13), (16, 16), (16, 20), (16, 40), (32, 40), (64, 80), (64, 64)]
BATCHES = [1, 2, 3, 4]
SPLITS = [0, 1, 3, 7]
N_FIT, N_OTHER = 60, 10          # draws per (kernel size, dtype, tune word), see rows()


def tune_words():
    from dyk import plan as P
    PS = 3 << 28
    words = [0] + list(P._WGRAD_CANDIDATES)
    # the words the GPU tests launch (tests/test_gpu_conv.py)
    words += [2 | (1 << 8) | (2 << 28), 2 | (2 << 8) | (2 << 28), 2 | (2 << 8) | (2 << 28) | (1 << 20), PS | 4 | (1 << 20)]
    words += [PS | ns for ns in (2, 3, 4, 6, 8)] + [PS | ns | (1 << 8) for ns in (2, 4)]
    words += [PS | ns | (1 << 8) | (1 << 12) for ns in (2, 4, 8)]
    return list(dict.fromkeys(words))


def make_desc(row):
    """DykWgradDesc of a table row (a dict over COLUMNS); keeps nothing alive: the queries read no tensor"""
    from dyk import lib as L
    from dyk.ops import fwd_taps
    d = L.DykWgradDesc()
    d.dtype = row["dtype"]
    epv = 8 if row["dtype"] == BF16 else 4
    d.B, d.Cin, d.Cout, d.Ho, d.Wo = row["B"], row["Cin"], row["Cout"], row["Ho"], row["Wo"]
    d.Hi, d.Wi = row["Ho"] * row["stride"], row["Wo"] * row["stride"]
    d.ldx, d.lddy = -(-row["Cin"] // epv) * epv, -(-row["Cout"] // epv) * epv
    d.isy = d.isx = row["stride"]
    taps = fwd_taps(row["k"], row["k"] // 2)
    d.ntaps = len(taps)
    for q, (ty, tx, wt) in enumerate(taps):
        d.tdy[q], d.tdx[q], d.twt[q] = ty, tx, wt
    d.tune, d.splits, d.lddw = row["tune"], row["splits"], 0
    if row["part"]:
        d.part, d.part_stride = 16, d.ntaps * d.Cout * d.Cin      # (the queries read only part's NULL-ness)
    return d


def answers(lib, row):
    d = make_desc(row)
    nt = ctypes.c_int32(-7)
    fold = int(lib.dyk_conv_wgrad_fold_ws_bytes(ctypes.byref(d), ctypes.byref(nt)))
    return [int(lib.dyk_conv_wgrad_splits(ctypes.byref(d))), int(lib.dyk_conv_wgrad_variant(ctypes.byref(d))), fold, nt.value]


def rows():
    out = []
    with open(os.path.join(ROOT, "bench_tuning.json")) as f:
        choices = json.load(f)["choices"]
    for key, ((tune, splits), _t) in ((ast.literal_eval(k), v) for k, v in choices.items() if k.startswith("('w'")):
        _, dtype, B, Cin, Cout, Ho, Wo, ntaps, isy = key
        for part in (0, 1):
            out.append(dict(dtype=dtype, B=B, Cin=Cin, Cout=Cout, Ho=Ho, Wo=Wo, k={1: 1, 9: 3}[ntaps], stride=isy, tune=tune,
                            splits=splits, part=part))
    n_bench = len(out)
    words = tune_words()
    rng = random.Random(20240)
    seen = set()
    # per (kernel size, dtype, tune word) a fixed number of draws of the other factors: most where the word's kernel variant can
    # apply to the kernel size (else the row only shows the fall-back to the per-tap kernel)
    for ks, dtype, tune in itertools.product(KERNELS, (BF16, F32), words):
        variant = (tune >> 28) & 7
        fits = dtype == BF16 and (ks == (1, 1) if variant == 3 else ks[0] == 3 if variant in (1, 2) else False)
        want, group = (N_FIT if fits else N_OTHER), set()
        while len(group) < want:
            group.add((ks, dtype, rng.choice(CHANNELS), rng.choice(CHANNELS), rng.choice(MAPS), rng.choice(BATCHES), tune,
                       rng.choice(SPLITS), rng.choice((0, 1))))
        seen |= group
    grid = sorted(seen)
    # every value of every factor meets every kernel size (and every split count both plane modes)
    for col, values in ((1, (BF16, F32)), (2, CHANNELS), (3, CHANNELS), (4, MAPS), (5, BATCHES), (6, words), (7, SPLITS)):
        assert {(g[0], g[col]) for g in grid} == set(itertools.product(KERNELS, values)), col
    assert {(g[7], g[8]) for g in grid} == set(itertools.product(SPLITS, (0, 1)))
    for (k, s), dtype, Cin, Cout, (Ho, Wo), B, tune, splits, part in grid:
        out.append(dict(dtype=dtype, B=B, Cin=Cin, Cout=Cout, Ho=Ho, Wo=Wo, k=k, stride=s, tune=tune, splits=splits, part=part))
    return out, n_bench


def main():
    from dyk import lib as L
    lib = L.load()
    table, n_bench = rows()
    lines = [json.dumps([r[c] for c in COLUMNS] + answers(lib, r), separators=(",", ":")) for r in table]
    with open(OUT, "w") as f:
        f.write('{"library": "%s",\n "columns": %s,\n "bench_rows": %d,\n "rows": [\n' % (
            lib.dyk_build_sha().decode(), json.dumps(COLUMNS + ANSWERS), n_bench))
        f.write(",\n".join(lines))
        f.write("\n]}\n")
    print("%s: %d rows (%d of bench_tuning.json), library %s" % (OUT, len(table), n_bench, lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
