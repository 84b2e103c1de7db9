"""The case matrix of dyk_clahe / dyk_cutout_rects (tests/test_clahe_reference.py on the CPU, tests/test_gpu_clahe.py on the
GPU).  Seeded; the smallest shapes at which each thing can go wrong.  Shapes are H x W, grids (tiles_x, tiles_y).

A case is a dict: imgs uint8 [planes, H, W], clip_limit, grid.  `reference(name)` is the yardstick's answer
(tests/clahe_ref.py), computed once per process and shared; its arrays are read-only."""
import functools

import numpy as np

import clahe_ref


def _rng(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def noise(name, planes, H, W):
    return _rng(name).randint(0, 256, size=(planes, H, W)).astype(np.uint8)


def peaked(name, planes, H, W):
    """LWIR-like: nearly every pixel within a few grey levels of one value, a few hot outliers"""
    r = _rng(name)
    img = np.rint(r.normal(92.0, 2.5, size=(planes, H, W)))
    hot = r.rand(planes, H, W) < 0.01
    img[hot] = r.randint(150, 256, size=int(hot.sum()))
    return np.clip(img, 0, 255).astype(np.uint8)


def constant(planes, H, W, v=100):
    return np.full((planes, H, W), v, np.uint8)


def two_valued(H, W):
    img = np.zeros((1, H, W), np.uint8)
    img[0, :, W // 3:] = 255
    img[0, H // 2:, : W // 3] = 255
    return img


def _c(imgs, clip_limit, grid):
    return {"imgs": imgs, "clip_limit": clip_limit, "grid": grid}


CASES = {
    # geometry
    "8x8_g2": lambda n: _c(noise(n, 1, 8, 8), 1.0, (2, 2)),                       # no padding; 16-pixel tiles: clip floored to 1
    "10x13_g4": lambda n: _c(noise(n, 1, 10, 13), 1.0, (4, 4)),                   # padded on both axes
    "10x12_g4": lambda n: _c(noise(n, 1, 10, 12), 1.0, (4, 4)),                   # W divisible, H not: a full extra tiles_x
    "5x5_g4": lambda n: _c(noise(n, 1, 5, 5), 1.0, (4, 4)),                       # pad 3 of n - 1 = 4
    "5x5_g9": lambda n: _c(noise(n, 1, 5, 5), 1.0, (9, 9)),                       # pad 4 == n - 1: the reflection reaches index 0
    "6x14_g2": lambda n: _c(noise(n, 1, 6, 14), 1.0, (2, 2)),                     # area 21: float(21) * (255.0f / 21) > 255.0f
    "33x47_g1": lambda n: _c(noise(n, 1, 33, 47), 2.0, (1, 1)),
    "33x47_g16x3": lambda n: _c(noise(n, 1, 33, 47), 2.0, (16, 3)),
    "33x47_g8": lambda n: _c(noise(n, 1, 33, 47), 2.0, (8, 8)),
    # hand-worked tables (tests/test_clahe_reference.py)
    "const_tile16": lambda n: _c(constant(1, 8, 8), 1.0, (2, 2)),                 # residual 15, step 17
    "const_tile256": lambda n: _c(constant(1, 32, 32), 1.0, (2, 2)),              # residual 255, step 1
    "two_valued": lambda n: _c(two_valued(18, 20), 3.0, (4, 4)),
    # every loop more than once, on an unaligned row (W = 97: 25 x 25 tiles, pad 3 and a forced 4)
    "noise_96x97": lambda n: _c(noise(n, 1, 96, 97), 1.0, (4, 4)),
    "peaked_96x97": lambda n: _c(peaked(n, 1, 96, 97), 1.0, (4, 4)),
    # clip limits on 32 x 32 tiles (1024 pixels: clip 0 = off, 0 -> 1, 4, 8, 160), word-aligned rows
    "clip0": lambda n: _c(peaked("clip", 1, 64, 64), 0.0, (2, 2)),
    "clip0.01": lambda n: _c(peaked("clip", 1, 64, 64), 0.01, (2, 2)),
    "clip1": lambda n: _c(peaked("clip", 1, 64, 64), 1.0, (2, 2)),
    "clip2": lambda n: _c(peaked("clip", 1, 64, 64), 2.0, (2, 2)),
    "clip40": lambda n: _c(peaked("clip", 1, 64, 64), 40.0, (2, 2)),
    # plane indexing
    "planes7": lambda n: _c(noise(n, 7, 11, 20), 1.0, (4, 4)),
    "planes7_words": lambda n: _c(np.concatenate([noise(n, 4, 16, 24), peaked(n, 3, 16, 24)]), 4.0, (2, 2)),
    # the one full-size case: a KAIST plane at the reference's grid
    "full_512x640": lambda n: _c(peaked(n, 1, 512, 640), 1.0, (4, 4)),
}
SMALL = [n for n in CASES if n != "full_512x640"]

# (H, W, grid) that dyk_clahe refuses; null pointers and planes < 1 are tried by the suites directly
REFUSED = [
    (5, 5, (10, 10)),          # pad 5 > n - 1 = 4
    (4, 5, (4, 4)),            # H divisible: the forced pad 4 > 3
    (1, 7, (2, 1)),            # pad 1 on an axis of one pixel
    (8, 8, (0, 2)), (8, 8, (2, 0)), (8, 8, (17, 2)), (8, 8, (2, 17)), (8, 8, (-1, 2)),
    (0, 8, (1, 1)), (8, 0, (1, 1)),
    (4097, 4096, (1, 1)),      # area 2^24 + 4096
]


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name](name)
    c["imgs"].setflags(write=False)
    return c


COVERAGE = {}          # case name -> the yardstick's branch counters of that case (filled by reference())


@functools.lru_cache(maxsize=None)
def reference(name, mutant=None):
    c = case(name)
    clahe_ref.COUNTERS.clear()
    dst, luts = clahe_ref.clahe(c["imgs"], c["clip_limit"], c["grid"], mutant=mutant)
    if mutant is None:
        COVERAGE[name] = dict(clahe_ref.COUNTERS)
    dst.setflags(write=False)
    luts.setflags(write=False)
    return dst, luts


# ---------------------------------------------------------------------------------------------- cut-outs
def _cut_img(name, planes, H, W):
    img = noise(name, planes, H, W)
    img[img == 0] = 1                                            # a written 0 can be told from what was there
    return img


CUT_CASES = {
    # six planes of 20 x 30, two rectangle sets: clipped at every edge, empty, inverted, outside, overlapping
    "two_sets": lambda n: {
        "imgs": _cut_img(n, 6, 20, 30), "planes_per_set": 3, "value": 0,
        "rects": np.array([[[-5, 2, 4, 6], [25, 3, 40, 8], [10, -7, 15, 3], [12, 15, 18, 99], [5, 5, 5, 9], [9, 9, 4, 12],
                            [6, 8, 12, 12], [9, 10, 16, 14]],
                           [[0, 0, 30, 1], [29, 19, 30, 20], [31, 2, 35, 6], [3, 21, 9, 25], [-9, -9, 0, 0], [7, 7, 8, 7],
                            [2, 3, 7, 9], [4, 5, 11, 6]]], np.int32)},
    # one set for all planes, a value other than 0, a rectangle that is the whole image and more
    "one_set_value7": lambda n: {
        "imgs": _cut_img(n, 4, 9, 13), "planes_per_set": 4, "value": 7,
        "rects": np.array([[[1, 1, 3, 4], [11, 6, 13, 9]]], np.int32)},
    "whole_image": lambda n: {
        "imgs": _cut_img(n, 2, 7, 5), "planes_per_set": 1, "value": 255,
        "rects": np.array([[[-1, -1, 99, 99]], [[2, 2, 2, 2]]], np.int32)},
    # the reference's own boxes: 25 of them, 16 wide, on one 64 x 80 pair (three planes a set)
    "snow25": lambda n: {
        "imgs": _cut_img(n, 6, 64, 80), "planes_per_set": 3, "value": 0,
        "rects": np.stack([np.concatenate([xy, xy + 15], 1) for xy in
                           (_rng(n).randint(0, 70, size=(2, 25, 2)))]).astype(np.int32)},
}


@functools.lru_cache(maxsize=None)
def cut_case(name):
    c = CUT_CASES[name](name)
    c["imgs"].setflags(write=False)
    c["rects"].setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------- wrong kernels
# mutant of the yardstick (a plausible wrong kernel) -> a named case that tells it from the rule
WITNESS = {
    "contract": "33x47_g16x3",
    "round_half_up": "33x47_g8",
    "clamp_before_xa": "8x8_g2",
    "pad0_on_divisible_axis": "10x12_g4",
    "reflect_without_minus_1": "10x13_g4",
    "residual_without_step": "const_tile16",
    "clip_not_floored": "clip0.01",
    "inclusive_ends": "two_sets",
}


def flagged(mutant):
    """does the witness case tell the mutant from the rule?  (a mutant that is refused where the rule is not counts)"""
    name = WITNESS[mutant]
    if mutant == "inclusive_ends":
        c = cut_case(name)
        return not np.array_equal(clahe_ref.cutout(c["imgs"], c["rects"], c["planes_per_set"], c["value"], mutant=mutant),
                                  clahe_ref.cutout(c["imgs"], c["rects"], c["planes_per_set"], c["value"]))
    good = reference(name)
    try:
        bad = reference(name, mutant)
    except ValueError:
        return True
    return not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]))
