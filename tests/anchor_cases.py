"""The case matrix of the anchor-clustering tests: the smallest shapes at which each piece of dyk_anchor_assign,
dyk_anchor_median and dyk_anchor_fitness can go wrong, and the named cases that tell wrong readings of the rule apart
(tests/test_anchor_reference.py shows on the CPU that each does; tests/test_gpu_anchor_cluster.py runs all of them on the
device).  Shapes: N = 1 and N = K for EVERY K of the matrix (each cluster a single box; for K = 24 and 32 both histogram
launches of a median pass, clusters 0..15 and 16.., see one-member selections only), N around the wave (63, 64, 65), around
an assignment workgroup (257), several workgroups and fitness items (4099), one box past a fitness item (1025) and one box past the first row of 64 item partials of the fold (65537, the one
large case).  Everything is generated from fixed seeds; nothing here is derived from the code under test."""
import numpy as np

DTYPES = (np.float32, np.float64)
KS = (1, 2, 9, 24, 32)
NS = (1, 63, 64, 65, 257, 4099)          # and N = K for every K: sizes(k)
N_ITEM_EDGE = 1025            # one box past a fitness item of 1024
N_FOLD_EDGE = 65537           # one box past 64 items: the fold's lane 0 takes a second partial
GS = (1, 7, 64, 1000)
THR = 0.25


def sizes(k):
    """the N of the matrix for K = k: 1, K, 63, 64, 65, 257, 4099"""
    return tuple(sorted(set(NS + (k,))))


def boxes(n, dtype, seed=0):
    return np.exp(np.random.RandomState(seed).randn(n, 2) * 0.6 + 3.3).astype(dtype)


def integer_boxes(n, dtype, seed=0, lo=2, hi=12):
    """integer sides with many duplicates: ties in d and equal middle elements"""
    return np.random.RandomState(seed).randint(lo, hi, size=(n, 2)).astype(dtype)


def centres(wh, k, seed=1):
    """k distinct rows of wh as initial centres"""
    return wh[np.random.RandomState(seed).choice(len(wh), k, replace=False)].copy()


def assign_cases():
    """name -> (wh, c): one assignment / median step each"""
    out = {}
    for T in DTYPES:
        t = T.__name__
        for k in KS:
            for n in sizes(k):
                if k <= n:
                    wh = boxes(n, T, seed=n)
                    out["random_N%d_K%d_%s" % (n, k, t)] = (wh, centres(wh, k))
        for n, k in ((64, 2), (257, 9), (4099, 32)):
            wh = integer_boxes(n, T, seed=n)
            # centres drawn from the distinct boxes, so that ties come from the boxes and not from equal centres
            uniq = np.unique(wh, axis=0)
            out["integer_N%d_K%d_%s" % (n, k, t)] = (wh, centres(uniq, k))
        for name, (wh, c) in named_cases(T).items():
            out["%s_%s" % (name, t)] = (wh, c)
    return out


def named_cases(T):
    """The hand-made cases, in type T.  name -> (wh, c)"""
    out = {}
    # two equal initial centres: every tie goes to the first, the second gets no member (the empty-cluster rule)
    wh = integer_boxes(65, T, seed=3)
    out["equal_centres"] = (wh, np.array([[4, 4], [9, 9], [9, 9], [6, 3]], T))
    # every box is nearest centre 0 on the first pass: changed == 0 against the zero-filled buffer
    out["all_cluster0"] = (boxes(65, T, seed=4), np.array([[27, 27], [4000, 4000], [9000, 2]], T))
    # iou 1.0e-8 and 1.8e-8 (fp32) / 1e-17 and 1.8e-17 (fp64): both 1 - iou round to 1, a tie that iou does not have
    s = T(1e4) if T is np.float32 else T(2e8)
    out["rounding_tie"] = (np.array([[2, 2], [3, 1]], T), np.array([[2 * s, 2 * s], [1.5 * s, 1.5 * s]], T))
    # an even cluster whose two middle elements differ, and an odd one
    out["even_count"] = (np.array([[1, 7], [2, 5], [4, 6], [8, 8], [50, 50], [60, 70], [70, 60]], T), np.array([[3, 6], [60, 60]], T))
    # per coordinate, not the member of median area: members (1,10) (5,5) (10,1) -> (5,5); areas 10, 25, 10
    out["per_coordinate"] = (np.array([[1, 10], [5, 5], [10, 1]], T), np.array([[5, 5]], T))
    # a near tie that one unrounded product in the denominator decides the other way (found by a seeded CPU search over
    # centres with equal rounded and different exact areas; fp32: an exact FMA, fp64: a 64-bit-significand intermediate)
    if T is np.float32:
        wh = [[float.fromhex("0x1.279dccp+4"), float.fromhex("0x1.095646p+5")]]
        c = [[float.fromhex("0x1.3dba94p+4"), float.fromhex("0x1.144798p+5")], [float.fromhex("0x1.406322p+4"), float.fromhex("0x1.11fcbap+5")]]
    else:
        wh = [[float.fromhex("0x1.fb3763ab145c2p+4"), float.fromhex("0x1.c6ea49b36896ep+4")]]
        c = [[float.fromhex("0x1.09d48478b953cp+5"), float.fromhex("0x1.d4103acd8f98fp+4")],
             [float.fromhex("0x1.0ae36eea66b59p+5"), float.fromhex("0x1.d2351a6865322p+4")]]
    out["fma_denominator"] = (np.array(wh, T), np.array(c, T))
    return out


def kmeans_cases():
    """name -> (wh, initial centres): whole k-means runs"""
    out = {}
    for T in DTYPES:
        t = T.__name__
        out["random_N257_K9_%s" % t] = (boxes(257, T), centres(boxes(257, T), 9))
        out["random_N4099_K9_%s" % t] = (boxes(4099, T), centres(boxes(4099, T), 9))
        wh = integer_boxes(257, T, seed=8)
        out["integer_N257_K5_%s" % t] = (wh, centres(np.unique(wh, axis=0), 5))
        for k in KS:                                              # N = K: every cluster a single box
            wh = boxes(k, T, seed=k)
            out["random_N%d_K%d_%s" % (k, k, t)] = (wh, centres(wh, k))
        for name in ("equal_centres", "all_cluster0", "even_count"):
            out["%s_%s" % (name, t)] = named_cases(T)[name]
    return out


def candidates(k, g, seed=2):
    """[g, k, 2] fp64 anchor candidates around the boxes' scale, clipped at 2 as the evolution's are"""
    return np.exp(np.random.RandomState(seed).randn(g, k, 2) * 0.5 + 3.3).clip(min=2.0)


def fitness_cases():
    """name -> (wh, a[G,K,2], thr)"""
    out = {}
    for T in DTYPES:
        t = T.__name__
        for k in (1, 9, 32):
            for n in sizes(k) + (N_ITEM_EDGE,):
                out["random_N%d_K%d_G7_%s" % (n, k, t)] = (boxes(n, T, seed=n), candidates(k, 7, seed=k), THR)
        for g in GS:
            out["random_N257_K9_G%d_%s" % (g, t)] = (boxes(257, T), candidates(9, g), THR)
        out["random_N4099_K24_G64_%s" % t] = (boxes(4099, T), candidates(24, 64), THR)
        out["fold_edge_N%d_K2_G1_%s" % (N_FOLD_EDGE, t)] = (boxes(N_FOLD_EDGE, T, seed=6), candidates(2, 1), THR)
        for name, (wh, a, thr) in named_fitness_cases().items():
            out["%s_%s" % (name, t)] = (wh.astype(T), a, thr)
    return out


def named_fitness_cases():
    """hand-made, exact in fp32 and fp64.  name -> (wh, a[1,K,2], thr)"""
    out = {}
    # w / a == thr exactly (2 / 8 = 0.25): strictly above is required, so the first box does not count; the second does
    out["thr_exact"] = (np.array([[2, 2], [4, 4]], np.float64), np.array([[[8, 8]]], np.float64), 0.25)
    # 1 / (9 / 7) = 0.7777777777777777 but 7 / 9 = 0.7777777777777778: the second division is a rounding of its own
    out["double_rounding"] = (np.array([[9, 5]], np.float64), np.array([[[7, 5]]], np.float64), 0.25)
    # nothing is strictly above 1: every fitness is 0, so an accept rule with >= takes every generation
    out["flat_fitness"] = (boxes(65, np.float64, seed=9), candidates(3, 1, seed=9), 1.0)
    return out
