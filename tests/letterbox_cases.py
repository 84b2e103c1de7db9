"""The case matrix of dyk_resize_pad_pairs (tests/test_letterbox_reference.py on the CPU, tests/test_gpu_letterbox.py on the GPU).
Seeded noise plus a few structured images; the smallest shapes at which each thing can go wrong.  Shapes are h x w.

A case is a dict: v, l lists of B uint8 source images ([3,h,w] for layout "chw", [h,w,3] for "hwc_bgr"); geom [B] of
(nh, nw, top, left, interp); out_size (Ho, Wo); layout; color.  `reference(name)` is the yardstick's answer
(tests/letterbox_ref.py), computed once per process and shared; its arrays are read-only.

The kernel stages the source rows of a band of 8 output rows in 32 KiB of LDS when they fit and reads global memory when they
do not: the `unstaged_*` cases are the smallest that take the second path (more than 32 KiB of source rows behind one band)."""
import functools

import numpy as np

import letterbox_ref as R

LIN, AREA = R.LINEAR, R.AREA

# found by search (tests/test_letterbox_reference.py: search_scale_pair, search_edge_sum) and hard-coded
SCALE_PAIR = (5845, 8192)                    # n_src, n_dst with 1 / (n_dst / n_src) != n_src / n_dst in fp64, and a LINEAR output that shows it
EDGE_SUM = (1, 5463)                         # n_src, n_dst with a right-edge column whose unreset a0 + a1 != 2048


def _rng(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def noise(name, shapes, layout="chw"):
    """two streams of noise images of the given (h, w); the second stream differs from the first"""
    r = _rng(name)
    mk = lambda h, w: r.randint(0, 256, size=(3, h, w) if layout == "chw" else (h, w, 3)).astype(np.uint8)
    return [mk(h, w) for h, w in shapes], [mk(h, w) for h, w in shapes]


def _c(src, geom, out_size, layout="chw", color=(0, 0, 0)):
    return {"v": src[0], "l": src[1], "geom": [tuple(g) for g in geom], "out_size": out_size, "layout": layout, "color": color}


def _one(name, h, w, nh, nw, interp, top=0, left=0, out_size=None, layout="chw", color=(0, 0, 0)):
    return _c(noise(name, [(h, w)], layout), [(nh, nw, top, left, interp)], out_size or (nh + top, nw + left), layout, color)


def _ramp(h, w):
    """a structured image: plane 0 a horizontal ramp, plane 1 a vertical one, plane 2 a checkerboard of 0 and 255"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) % 2) * 255]).astype(np.uint8)


def _eps_row():
    """1 x 4001 for AREA -> 1 x 2000: scale 2.0005, so column 0 has f2 - s2 = 0.0005 <= 1e-3 and its third tap is dropped.
    Bytes 255, 0, 255 make (255 + 0) / 2.0005 = 127.47 -> 127 with the rule and 127.53 -> 128 with the tap kept"""
    r = _rng("eps_row")
    v, l = (r.randint(0, 256, size=(3, 1, 4001)).astype(np.uint8) for _ in range(2))
    for a in (v, l):
        a[:, 0, 0:3] = (255, 0, 255)
    return [v], [l]


CASES = {
    # identity: pad only, odd pad (top != bottom, left != right), non-zero colours
    "pad_only_odd": lambda n: _one(n, 9, 13, 9, 13, LIN, top=2, left=3, out_size=(14, 20), color=(10, 128, 250)),
    "copy_w37": lambda n: _one(n, 11, 37, 11, 37, AREA, top=0, left=0, out_size=(11, 37)),
    # 5:4 shrink in both modes
    "shrink54_lin_15x20": lambda n: _one(n, 15, 20, 12, 16, LIN, top=2, left=0, out_size=(16, 16)),
    "shrink54_area_15x20": lambda n: _one(n, 15, 20, 12, 16, AREA, top=2, left=0, out_size=(16, 16)),
    "shrink54_lin_20x25": lambda n: _one(n, 20, 25, 16, 20, LIN, top=1, left=3, out_size=(19, 27), color=(7, 7, 7)),
    "shrink54_area_20x25": lambda n: _one(n, 20, 25, 16, 20, AREA, top=1, left=3, out_size=(19, 27)),
    "ramp_area_20x25": lambda n: _c(([_ramp(20, 25)], [_ramp(20, 25)[::-1].copy()]), [(16, 20, 0, 0, AREA)], (16, 20)),
    # upscale: sy = -1 at the top, sx + 1 >= w on the right
    "up_9x13": lambda n: _one(n, 9, 13, 22, 31, LIN, top=1, left=0, out_size=(24, 32)),
    "ramp_up_9x13": lambda n: _c(([_ramp(9, 13)], [_ramp(9, 13)[::-1].copy()]), [(22, 31, 0, 0, LIN)], (22, 31)),
    # exact factors
    "exact2_lin": lambda n: _one(n, 12, 16, 6, 8, LIN),
    "exact2_area": lambda n: _one(n, 12, 16, 6, 8, AREA),
    "area3": lambda n: _one(n, 12, 18, 4, 6, AREA, top=1, left=1, out_size=(6, 8)),
    "area3x2": lambda n: _one(n, 8, 18, 4, 6, AREA),                       # kx = 3, ky = 2
    "area1x2": lambda n: _one(n, 8, 7, 4, 7, AREA),                        # one axis stays
    # steep fractional AREA: many taps
    "area_123x150": lambda n: _one(n, 123, 150, 100, 121, AREA),           # enough pixels for the rare roundings a fused multiply-add changes
    "steep_area_64": lambda n: _one(n, 64, 64, 3, 5, AREA, top=2, left=1, out_size=(7, 7)),
    "area_one_axis": lambda n: _one(n, 17, 9, 11, 9, AREA),                # weighted, nw == w
    # degenerate sizes
    "src_1x1": lambda n: _one(n, 1, 1, 5, 7, LIN, top=1, left=1, out_size=(7, 9), color=(1, 2, 3)),
    "out_1wide": lambda n: _one(n, 9, 13, 6, 1, AREA, top=0, left=2, out_size=(6, 5)),
    "out_1high": lambda n: _one(n, 9, 13, 1, 8, LIN, top=3, left=0, out_size=(5, 8)),
    # odd widths (byte stores, misaligned staging)
    "lin_w13": lambda n: _one(n, 10, 13, 7, 9, LIN, top=0, left=2, out_size=(7, 13)),
    "area_w37": lambda n: _one(n, 21, 37, 13, 30, AREA, top=1, left=3, out_size=(15, 37)),
    # the interleaved layout, channels reversed
    "hwc_copy": lambda n: _one(n, 7, 10, 7, 10, LIN, top=1, left=1, out_size=(9, 12), layout="hwc_bgr", color=(10, 128, 250)),
    "hwc_lin_w13": lambda n: _one(n, 10, 13, 8, 10, LIN, top=0, left=1, out_size=(8, 12), layout="hwc_bgr"),
    "hwc_area_w37": lambda n: _one(n, 21, 37, 13, 30, AREA, top=1, left=3, out_size=(15, 37), layout="hwc_bgr"),
    "hwc_area3": lambda n: _one(n, 12, 18, 4, 6, AREA, layout="hwc_bgr"),
    "hwc_up_9x13": lambda n: _one(n, 9, 13, 22, 31, LIN, layout="hwc_bgr"),
    # three images of three sizes, mixed interp, one launch; more than one band
    "batch3_mixed": lambda n: _c(noise(n, [(15, 20), (24, 32), (12, 16)]), [(12, 16, 4, 2, AREA), (18, 20, 1, 0, LIN), (12, 16, 4, 2, LIN)],
                                 (20, 20), color=(114, 114, 114)),
    "hwc_batch3_mixed": lambda n: _c(noise(n, [(15, 20), (24, 32), (12, 16)], "hwc_bgr"), [(12, 16, 4, 2, AREA), (12, 16, 0, 4, AREA),
                                                                                         (20, 20, 0, 0, LIN)], (20, 20), "hwc_bgr"),
    # bands whose source rows do not fit the LDS stage: taps read from global memory
    "unstaged_area": lambda n: _one(n, 200, 300, 3, 7, AREA),
    "unstaged_area_int": lambda n: _one(n, 201, 300, 3, 3, AREA),
    "unstaged_linear": lambda n: _one(n, 120, 700, 6, 35, LIN, layout="hwc_bgr"),
    # the rules that only special sizes separate
    "eps_4001": lambda n: _c(_eps_row(), [(1, 2000, 0, 0, AREA)], (1, 2000)),
    "tie_3_to_2048": lambda n: _one(n, 1, 3, 1, 2048, LIN),                # every fx * 2048 is k + 0.5
    "scale_pair": lambda n: _one(n, 1, SCALE_PAIR[0], 1, SCALE_PAIR[1], LIN),
    "edge_sum": lambda n: _one(n, 6, EDGE_SUM[0], 15, EDGE_SUM[1], LIN),    # (rows enlarged too: both row coefficients at work)
    # one full-size batch: 16 pairs of 512 x 640 -> 410 x 512 content in 512 x 512, LINEAR and AREA alternating
    "full_512x640": lambda n: _c(noise(n, [(512, 640)] * 16), [(410, 512, 51, 0, b % 2) for b in range(16)], (512, 512), color=(114, 114, 114)),
}
FULL = "full_512x640"
SMALL = [n for n in CASES if n != FULL]

# each wrong kernel of letterbox_ref.MUTANTS and the case that flags it
MUTANT_CASE = {
    "shift22": "up_9x13",
    "scale_src_over_dst": "scale_pair",
    "no_edge_exception": "edge_sum",
    "fy_reset_top": "up_9x13",
    "half_away": "tie_3_to_2048",
    "area2_float": "exact2_area",
    "area_fma": "area_123x150",
    "no_eps": "eps_4001",
    "pad_off_by_one": "pad_only_odd",
    "no_channel_reverse": "hwc_lin_w13",
    "swap_top_left": "pad_only_odd",
    "linear2x_not_switched": "exact2_lin",
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name](name)
    for a in c["v"] + c["l"]:
        a.setflags(write=False)
    return c


def run_ref(name, mutant=None):
    c = case(name)
    return R.resize_pad(c["v"], c["l"], c["geom"], c["out_size"], c["layout"], c["color"], mutant=mutant)


@functools.lru_cache(maxsize=None)
def reference(name):
    ov, ol = run_ref(name)
    ov.setflags(write=False)
    ol.setflags(write=False)
    return ov, ol
