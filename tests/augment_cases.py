"""The case matrix of dyk_augment_pairs (tests/test_augment_reference.py on the CPU, tests/test_gpu_augment.py on the GPU).
Seeded; the smallest shapes at which each thing can go wrong.  Shapes are H x W.

A case is a dict: src_v, src_l uint8 [N,3,H,W]; B; M forward matrices fp64 [B,2,3] or None; rects int32 [B,4,8] with canvas
(Hc, Wc), or None; out_size (Ho, Wo) or None; luts uint8 [B,3,256] or None; flip uint8 [B] or None; in_place; raw (a case only
the C entry admits: the Python wrapper refuses it).  `reference(name)` is the yardstick's answer (tests/augment_ref.py),
computed once per process and shared; its arrays are read-only."""
import functools
import math

import numpy as np

import augment_ref

HYP_GAINS = (0.0138, 0.678, 0.36)            # hsv_h, hsv_s, hsv_v of config/hyp.scratch.json


def _rng(name):
    return np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))


def noise(name, N, H, W):
    """two streams of smooth-free noise; the second differs from the first"""
    r = _rng(name)
    return r.randint(0, 256, size=(N, 3, H, W)).astype(np.uint8), r.randint(0, 256, size=(N, 3, H, W)).astype(np.uint8)


def rot(deg, scale, cx, cy):
    """the rotation matrix about (cx, cy) as the rule's host half writes it out"""
    a = deg * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy], [0, 0, 1]])


def shift(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1]])


def shear(dx, dy):
    return np.array([[1.0, math.tan(dx * math.pi / 180), 0], [math.tan(dy * math.pi / 180), 1.0, 0], [0, 0, 1]])


def tables(*draws, gains=(0.5, 0.5, 0.5)):
    """tables of the given uniform(-1, 1, 3) draws"""
    return np.stack([augment_ref.hsv_tables(np.asarray(d, np.float64) * list(gains) + 1) for d in draws])


IDENTITY_TABLE = np.stack([np.arange(256) % 180, np.arange(256), np.arange(256)]).astype(np.uint8)


def _c(src, B=None, M=None, rects=None, canvas=None, out_size=None, luts=None, flip=None, in_place=False, raw=False):
    v, l = src
    B = v.shape[0] if B is None else B
    if M is not None:
        M = np.asarray(M, np.float64)
        M = np.stack([m[:2] for m in (M if M.ndim == 3 else [M] * B)])
    return {"src_v": v, "src_l": l, "B": B, "M": M, "rects": None if rects is None else np.asarray(rects, np.int32), "canvas": canvas,
            "out_size": out_size, "luts": luts, "flip": None if flip is None else np.asarray(flip, np.uint8), "in_place": in_place,
            "raw": raw}


def quad_rects(xr, yr, s, h, w, srcs):
    """the four rectangles of a mosaic centred at (xr, yr) on a 2s x 2s canvas, tiles of h x w from the sources `srcs`
    (above-left, above-right, below-left, below-right; each tile touches the centre with one corner)"""
    out = []
    for i, j in enumerate(srcs):
        left, top = i % 2 == 0, i < 2
        x1, x2 = (max(xr - w, 0), xr) if left else (xr, min(xr + w, 2 * s))
        y1, y2 = (max(yr - h, 0), yr) if top else (yr, min(yr + h, 2 * s))
        dx = (x2 - w) if left else x1                            # canvas x - dx = source x
        dy = (y2 - h) if top else y1
        out.append((x1, y1, x2, y2, j, dx, dy, 0))
    return out


def lattice():
    """every combination of 32 levels per channel (all ties r == g, g == b, r == b, the greys, the extremes and their
    neighbours) as one 128 x 256 image, and 128 x 256 random colours with a band of random greys"""
    lv = np.array([0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 47, 63, 64, 65, 96, 100, 127, 128, 129, 150, 160, 191, 192, 200, 223, 224,
                   240, 250, 253, 254, 255], np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing="ij")
    v = np.stack([r.reshape(128, 256), g.reshape(128, 256), b.reshape(128, 256)])[None]
    rnd = _rng("lattice").randint(0, 256, size=(1, 3, 128, 256)).astype(np.uint8)
    rnd[0, :, :8] = rnd[0, 0, :8]
    return v, rnd


def _mosaic_case(n, xr, yr, M=None, **kw):
    s, h, w = 16, 12, 16
    if M is None:
        M = shift(-8, -8) @ rot(7, 1.1, 16, 16)
    return _c(noise(n, 4, h, w), B=1, M=M, rects=[quad_rects(xr, yr, s, h, w, (0, 3, 1, 2))], canvas=(32, 32), out_size=(16, 16), **kw)


CASES = {
    # the hand-worked cases of the rule (tests/test_augment_reference.py holds their literals)
    "id_8x8": lambda n: _c(noise(n, 1, 8, 8), M=np.eye(3)),
    "shift_8x8": lambda n: _c(noise(n, 1, 8, 8), M=shift(2, 1)),
    "half_8x8": lambda n: _c(noise(n, 1, 8, 8), M=shift(0.5, 0)),
    "rot90_8x8": lambda n: _c(noise(n, 1, 8, 8), M=rot(90, 1.0, 4, 4)),
    "crop_8x8": lambda n: _c(noise(n, 1, 8, 8), M=shift(-2, -2), out_size=(4, 4)),
    # geometry
    "general_9x13": lambda n: _c(noise(n, 1, 9, 13), M=shear(3, -2) @ shift(0.7, -1.3) @ rot(13, 0.93, 6.5, 4.5)),
    "edges_9x13": lambda n: _c(noise(n, 1, 9, 13), M=shift(2.6, 1.4), out_size=(13, 18)),      # taps at -1.. and past both far edges
    "general_37x53": lambda n: _c(noise(n, 1, 37, 53), M=shift(1.25, -2.5) @ rot(-6, 1.05, 26.5, 18.5)),   # Wo % 4 == 1, many strips
    "to_11x10": lambda n: _c(noise(n, 1, 9, 13), M=rot(4, 0.9, 6.5, 4.5), out_size=(11, 10)),   # Ho != Wo != H != W
    "scale_0p5": lambda n: _c(noise(n, 1, 16, 20), M=rot(0, 0.5, 10, 8)),
    "scale_1p5": lambda n: _c(noise(n, 1, 16, 20), M=rot(0, 1.5, 10, 8)),
    "rot10_shear10": lambda n: _c(noise(n, 1, 24, 28), M=shear(10, 10) @ rot(10, 1.0, 14, 12)),
    "crop_64": lambda n: _c(noise(n, 1, 64, 64), M=shift(-16, -16) @ rot(5, 0.95, 32, 32), out_size=(32, 32)),   # border = -16
    # the virtual canvas
    "canvas4_mid": lambda n: _mosaic_case(n, 16, 16),
    "canvas4_low": lambda n: _mosaic_case(n, 8, 8),               # centre at 0.5 s: the left and top tiles are cut, corners empty
    "canvas4_high": lambda n: _mosaic_case(n, 23, 23),            # centre at int(1.5 s - eps)
    "canvas4_seams": lambda n: _mosaic_case(n, 15, 17, M=shift(-8.3, -7.6)),   # axis-parallel, every row and column crosses a seam
    "canvas4_no_matrix": lambda n: _c(noise(n, 4, 12, 16), B=1, rects=[quad_rects(13, 18, 16, 12, 16, (2, 0, 3, 1))], canvas=(32, 32)),
    "canvas_clipped": lambda n: _c(noise(n, 2, 8, 8), B=1, M=shift(0.5, 0.5), rects=[[(6, 6, 14, 14, 1, 6, 6, 0), (0, 0, 0, 0, 0, 0, 0, 0),
                                   (-2, 0, 6, 6, 0, -2, -2, 0), (0, 0, 0, 0, 0, 0, 0, 0)]], canvas=(10, 10)),
    "rect_outside_source": lambda n: _c(noise(n, 2, 8, 8), B=1, rects=[[(0, 0, 8, 8, 0, 0, 0, 0), (8, 0, 16, 8, 1, 7, 0, 0),
                                        (0, 8, 8, 16, 2, 0, 8, 0), (8, 8, 16, 16, 1, 8, 8, 0)]], canvas=(16, 16), raw=True),
    # per-image parameters
    "batch3_picked": lambda n: _c(noise(n, 5, 10, 12), B=3, M=[rot(8, 1.0, 6, 5), shift(1.5, -0.5), rot(-15, 1.2, 6, 5)],
                                  rects=[[(0, 0, 12, 10, 4, 0, 0, 0)] + [(0,) * 8] * 3, [(0, 0, 12, 10, 2, 0, 0, 0)] + [(0,) * 8] * 3,
                                         [(0, 0, 12, 10, 0, 0, 0, 0)] + [(0,) * 8] * 3], canvas=(10, 12),
                                  luts=tables((0.3, -0.6, 0.9), (-0.9, 0.8, -0.4), (0.5, 0.1, 0.2)), flip=[1, 0, 1]),
    "batch3_plain": lambda n: _c(noise(n, 3, 10, 13), M=[rot(8, 1.0, 6.5, 5), shift(1.5, -0.5), rot(-15, 1.2, 6.5, 5)],
                                 luts=tables((0.3, -0.6, 0.9), (-0.9, 0.8, -0.4), (0.5, 0.1, 0.2)), flip=[0, 1, 1]),
    # stages alone and together
    "jitter_in_place": lambda n: _c(noise(n, 2, 9, 12), luts=tables((0.7, -0.2, 0.4), (-0.5, 0.9, -0.8)), in_place=True),
    "jitter_in_place_w13": lambda n: _c(noise(n, 2, 9, 13), luts=tables((0.7, -0.2, 0.4), (-0.5, 0.9, -0.8)), in_place=True),
    "flip_alone_w10": lambda n: _c(noise(n, 2, 7, 10), flip=[1, 0]),
    "flip_alone_w12": lambda n: _c(noise(n, 2, 7, 12), flip=[0, 1]),
    "flip_warp_9x13": lambda n: _c(noise(n, 1, 9, 13), M=shift(1.5, 0), flip=[1]),
    "all_stages": lambda n: _c(noise(n, 4, 12, 16), B=2, M=[shift(-8, -8) @ shear(2, -3) @ rot(9, 0.9, 16, 16), shift(-6.5, -9) @ rot(-4, 1.1, 16, 16)],
                               rects=[quad_rects(14, 19, 16, 12, 16, (0, 1, 2, 3)), quad_rects(20, 11, 16, 12, 16, (1, 1, 3, 0))],
                               canvas=(32, 32), out_size=(16, 16), luts=tables((0.1, 0.5, -0.5), (-0.2, -0.7, 0.6)), flip=[1, 0]),
    # HSV on its own: every tie, the greys and the extremes
    "hsv_identity_table": lambda n: _c(lattice(), luts=IDENTITY_TABLE[None]),
    "hsv_hyp_gains": lambda n: _c(lattice(), luts=tables((1.0, -1.0, 1.0), gains=HYP_GAINS)),
    # tables that send every pixel to (1, 15, 255) and (3, 15, 85): channels of exactly 240.5 and 80.5, ties of the final rounding
    "hsv_exact_tie": lambda n: _c(noise(n, 2, 5, 6), luts=np.stack([np.repeat(np.array([[1], [15], [255]], np.uint8), 256, 1),
                                                                  np.repeat(np.array([[3], [15], [85]], np.uint8), 256, 1)])),
    # one full-size batch
    "full_512x640": lambda n: _c(noise(n, 2, 512, 640), M=[shift(3.5, -7.25) @ rot(5, 0.9, 320, 256), rot(-10, 1.1, 320, 256)],
                                 luts=tables((0.4, -0.3, 0.8), (-0.6, 0.5, -0.2)), flip=[1, 0]),
}
FULL = "full_512x640"
SMALL = [n for n in CASES if n != FULL]


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name](name)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def minv(c):
    return None if c["M"] is None else np.stack([augment_ref.invert(m) for m in c["M"]])


def run_ref(name, mutant=None):
    c = case(name)
    return augment_ref.augment(c["src_v"], c["src_l"], c["B"], c["rects"], c["canvas"], minv(c), c["out_size"], c["luts"], c["flip"],
                               mutant=mutant)


@functools.lru_cache(maxsize=None)
def reference(name):
    ov, ol = run_ref(name)
    ov.setflags(write=False)
    ol.setflags(write=False)
    return ov, ol
