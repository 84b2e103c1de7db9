"""The yardstick of dyk_clahe and dyk_cutout_rects: a deliberately plain numpy restatement of the rule in include/dyk_hip.h
(OpenCV's 8-bit CLAHE, modules/imgproc/src/clahe.cpp).  Loops over tiles and pixels, np.float32 scalars, np.rint; nothing
here shares code with the kernels or their host code.  Written from the published algorithm: no OpenCV is installed where
this project runs, so agreement with it is derived, not measured.

COUNTERS records which branches of the rule a call went through; tests/test_clahe_reference.py asserts that the case matrix
(tests/clahe_cases.py) reaches every one.

`mutant=` selects one of the plausible wrong kernels (MUTANTS); the suites assert that each is told apart from the rule by a
named case, i.e. that the cases would catch a kernel that made that mistake."""
import collections

import numpy as np

F = np.float32
COUNTERS = collections.Counter()
COUNTER_NAMES = (
    "pad_none", "pad_both", "pad_forced_on_divisible_axis", "clip_zero", "clip_floored_to_1", "residual_zero", "step_one",
    "step_above_one", "saturate_255", "band_left", "band_right", "band_top", "band_bottom")
MUTANTS = ("contract", "round_half_up", "clamp_before_xa", "pad0_on_divisible_axis", "reflect_without_minus_1",
           "residual_without_step", "clip_not_floored")          # + "inclusive_ends" of cutout()


def geometry(H, W, tiles_x, tiles_y, mutant=None):
    """-> (padx, pady, tw, th), or ValueError for what dyk_clahe refuses"""
    if H < 1 or W < 1 or not (1 <= tiles_x <= 16) or not (1 <= tiles_y <= 16):
        raise ValueError("shape or grid out of range")
    if W % tiles_x == 0 and H % tiles_y == 0:
        padx = pady = 0
        COUNTERS["pad_none"] += 1
    else:
        padx = tiles_x - W % tiles_x
        pady = tiles_y - H % tiles_y
        if W % tiles_x == 0 or H % tiles_y == 0:
            COUNTERS["pad_forced_on_divisible_axis"] += 1
            if mutant == "pad0_on_divisible_axis":
                padx = padx if W % tiles_x else 0
                pady = pady if H % tiles_y else 0
        else:
            COUNTERS["pad_both"] += 1
    if padx > W - 1 or pady > H - 1:
        raise ValueError("pad larger than n - 1: the reflection is undefined")
    tw, th = (W + padx) // tiles_x, (H + pady) // tiles_y
    if tw * th > 2 ** 24:
        raise ValueError("tile area above 2^24")
    return padx, pady, tw, th


def _reflect(j, n, mutant=None):
    if j < n:
        return j
    return 2 * n - 1 - j if mutant == "reflect_without_minus_1" else 2 * (n - 1) - j


def _round_u8(v, mutant=None):
    """saturate_u8(rint_half_even(v)) of an np.float32.  saturate_255 counts the values above 255.0f that arrive here: fp32
    rounding puts (float)area * (255.0f / area) there for some areas (21 is the smallest)"""
    if v > F(255.0):
        COUNTERS["saturate_255"] += 1
    r = np.floor(v + F(0.5)) if mutant == "round_half_up" else np.rint(v)
    return np.uint8(min(max(int(r), 0), 255))


def tile_table(hist, area, clip_limit, mutant=None):
    """steps 2 and 3 of the rule on one 256-bin histogram (python ints) -> uint8[256]"""
    h = [int(v) for v in hist]
    clip = 0
    if clip_limit > 0:
        clip = int(float(clip_limit) * float(area) / 256.0)
        if clip < 1:
            COUNTERS["clip_floored_to_1"] += 1
            clip = 0 if mutant == "clip_not_floored" else 1
        clip = min(clip, 2 ** 31 - 1)
    else:
        COUNTERS["clip_zero"] += 1
    if clip > 0 or (clip_limit > 0 and mutant == "clip_not_floored"):
        clipped = 0
        for i in range(256):
            if h[i] > clip:
                clipped += h[i] - clip
                h[i] = clip
        batch = clipped // 256
        residual = clipped - 256 * batch
        for i in range(256):
            h[i] += batch
        if residual != 0:
            step = max(256 // residual, 1)
            COUNTERS["step_one" if step == 1 else "step_above_one"] += 1
            if mutant == "residual_without_step":
                step = 1
            i = 0
            while i < 256 and residual > 0:
                h[i] += 1
                i += step
                residual -= 1
        else:
            COUNTERS["residual_zero"] += 1
    lut_scale = F(255.0) / F(area)
    lut = np.zeros(256, np.uint8)
    s = 0
    for i in range(256):
        s += h[i]
        lut[i] = _round_u8(F(s) * lut_scale, mutant)
    return lut


def _fma(a, b, c):
    """a * b + c rounded once (through fp64: the product of two fp32 is exact there)"""
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def _axis_weights(i, inv, ntiles, mutant=None):
    """-> (t1, t2, a, a1) of pixel index i along one axis; also says whether a clamp bit"""
    tf = _fma(F(i), inv, F(-0.5)) if mutant == "contract" else F(i) * inv - F(0.5)
    t1 = int(np.floor(tf))
    if mutant == "clamp_before_xa":
        t1 = max(t1, 0)
    a = tf - F(t1)
    a1 = F(1.0) - a
    t2 = t1 + 1
    lo, hi = t1 < 0, t2 > ntiles - 1
    return max(t1, 0), min(t2, ntiles - 1), a, a1, lo, hi


def clahe_plane(src, clip_limit=1.0, tile_grid_size=(4, 4), mutant=None):
    """one uint8 plane [H, W] -> (dst uint8 [H, W], tables uint8 [tiles_y*tiles_x, 256])"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    H, W = src.shape
    tiles_x, tiles_y = int(tile_grid_size[0]), int(tile_grid_size[1])
    padx, pady, tw, th = geometry(H, W, tiles_x, tiles_y, mutant)
    area = tw * th
    luts = np.zeros((tiles_y * tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                ry = _reflect(y, H, mutant)
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[src[ry, _reflect(x, W, mutant)]] += 1
            luts[ty * tiles_x + tx] = tile_table(hist, area, clip_limit, mutant)
    inv_tw, inv_th = F(1.0) / F(tw), F(1.0) / F(th)
    dst = np.zeros_like(src)
    xs = [_axis_weights(x, inv_tw, tiles_x, mutant) for x in range(W)]
    for y in range(H):
        ty1, ty2, ya, ya1, top, bottom = _axis_weights(y, inv_th, tiles_y, mutant)
        COUNTERS["band_top"] += int(top)
        COUNTERS["band_bottom"] += int(bottom)
        for x in range(W):
            tx1, tx2, xa, xa1, left, right = xs[x]
            if y == 0:
                COUNTERS["band_left"] += int(left)
                COUNTERS["band_right"] += int(right)
            v = src[y, x]
            l11, l12 = F(luts[ty1 * tiles_x + tx1, v]), F(luts[ty1 * tiles_x + tx2, v])
            l21, l22 = F(luts[ty2 * tiles_x + tx1, v]), F(luts[ty2 * tiles_x + tx2, v])
            if mutant == "contract":
                res = _fma(_fma(l12, xa, l11 * xa1), ya1, _fma(l22, xa, l21 * xa1) * ya)
            else:
                res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya
            dst[y, x] = _round_u8(res, mutant)
    return dst, luts


def clahe(imgs, clip_limit=1.0, tile_grid_size=(4, 4), mutant=None):
    """uint8 [..., H, W] -> (dst of the same shape, tables [planes, tiles_y*tiles_x, 256])"""
    imgs = np.asarray(imgs)
    planes = imgs.reshape((-1,) + imgs.shape[-2:])
    out = [clahe_plane(p, clip_limit, tile_grid_size, mutant) for p in planes]
    return np.stack([o[0] for o in out]).reshape(imgs.shape), np.stack([o[1] for o in out])


def cutout(imgs, rects, planes_per_set, value=0, mutant=None):
    """uint8 [planes, H, W], int rects [nsets, nrect, 4] = (xmin, ymin, xmax, ymax) -> a cut copy: plane p takes set
    p // planes_per_set; rows [ymin, ymax), columns [xmin, xmax), clipped to the image; empty and inverted write nothing"""
    out = np.array(imgs, copy=True)
    P, H, W = out.shape
    e = 1 if mutant == "inclusive_ends" else 0
    for p in range(P):
        for xmin, ymin, xmax, ymax in np.asarray(rects)[p // planes_per_set]:
            x0, y0, x1, y1 = max(int(xmin), 0), max(int(ymin), 0), min(int(xmax) + e, W), min(int(ymax) + e, H)
            if x1 > x0 and y1 > y0:
                out[p, y0:y1, x0:x1] = value
    return out
