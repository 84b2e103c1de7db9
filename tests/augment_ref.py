"""The yardstick of dyk_augment_pairs: a deliberately plain numpy restatement of the rule in include/dyk_hip.h -- the virtual
canvas, the fp64 inversion, the fixed-point bilinear warp, RGB -> HSV -> tables -> RGB, the flipped store.  Whole-image numpy
arrays, np.float64 / np.float32 elementwise operations (each rounded on its own), np.rint; nothing here shares code with the
kernel or its host code.  The rule is the classical OpenCV 8-bit path written down as this project's own: no OpenCV is
installed where this project runs, so agreement with it is derived, not measured.

COUNTERS records which branches of the rule a call went through; tests/test_augment_reference.py asserts that the case matrix
(tests/augment_cases.py) reaches every one.

`mutant=` selects one of the plausible wrong kernels (MUTANTS); the suites assert that each is told apart from the rule by a
named case, i.e. that the cases would catch a kernel that made that mistake."""
import collections

import numpy as np

F = np.float32
COUNTERS = collections.Counter()
COUNTER_NAMES = (
    "rects_plain", "rects_listed", "rect_unused_slot", "rect_clipped_to_canvas", "rect_skipped_outside_source",
    "warp_null", "warp_matrix", "tap_negative", "tap_outside_every_rect", "quad_in_one_rect", "quad_straddles_rects",
    "quad_partly_empty", "fraction_zero", "fraction_nonzero",
    "jitter_none", "hsv_v_is_r", "hsv_v_is_g", "hsv_v_is_b", "hsv_h_wrapped", "hsv_grey", "hsv_exact_tie",
    "hsv_sector_0", "hsv_sector_1", "hsv_sector_2", "hsv_sector_3", "hsv_sector_4", "hsv_sector_5",
    "flip_none", "flip_yes", "flip_no")
MUTANTS = ("truncate", "replicate_border", "no_plus_16", "div_not_shift", "no_h_plus_180", "sector_row_permuted",
           "lut0_for_all", "l_wrong_matrix", "flip_source_side", "swap_HoWo", "seam_first_rect", "round_half_away")
# round_half_away is here because exact ties exist: (h, s, v) = (1, 15, 255) gives a channel of exactly 240.5
# (tests/test_augment_reference.py searches all triples).  One more that no case CAN flag, asserted there too: "g_before_r"
# (with v == r == g the two hue branches give the same number, diff; likewise with g == b).

SECTOR_TAB = ((1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0))      # (b, g, r) indices into tab, per sector


def invert(M):
    """forward 2 x 3 (or 3 x 3) matrix -> the six fp64 numbers of the inverse map, in the order of the rule"""
    m = [np.float64(M[0][0]), np.float64(M[0][1]), np.float64(M[0][2]), np.float64(M[1][0]), np.float64(M[1][1]), np.float64(M[1][2])]
    D = m[0] * m[4] - m[1] * m[3]
    if not np.isfinite(D) or D == 0:
        raise ValueError("singular or non-finite matrix")
    D = np.float64(1.0) / D
    A11 = m[4] * D
    A22 = m[0] * D
    m[0] = A11
    m[1] = m[1] * -D
    m[3] = m[3] * -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1
    m[5] = b2
    return np.array(m, np.float64)


def _rn(v):
    """round half to even to int32; saturation never happens in an admitted call, and the yardstick insists on that"""
    r = np.rint(np.asarray(v, np.float64))
    assert np.all(np.abs(r) < 2.0 ** 31), "an admitted call never saturates"
    return r.astype(np.int64)


def div_tables():
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, np.int64)
    hdiv = np.zeros(256, np.int64)
    sdiv[1:] = _rn(np.float64(255 << 12) / (1.0 * i))
    hdiv[1:] = _rn(np.float64(180 << 12) / (6.0 * i))
    return sdiv, hdiv


def _shift(v, n, mutant):
    """v >> n, arithmetic (numpy's >> on signed integers is)"""
    if mutant == "div_not_shift":
        return np.trunc(v / float(1 << n)).astype(np.int64)
    return v >> n


def warp_coords(m, Ho, Wo, mutant=None):
    """(b) up to the taps: -> sx, sy, fx, fy, int64 [Ho, Wo]"""
    m = np.asarray(m, np.float64)
    x = np.arange(Wo, dtype=np.float64)
    y = np.arange(Ho, dtype=np.float64)
    k = np.float64(1024.0)
    ad = _rn(m[0] * x * k)
    bd = _rn(m[3] * x * k)
    plus = 0 if mutant == "no_plus_16" else 16
    X0 = _rn((m[1] * y + m[2]) * k) + plus
    Y0 = _rn((m[4] * y + m[5]) * k) + plus
    X = _shift(X0[:, None] + ad[None, :], 5, mutant)
    Y = _shift(Y0[:, None] + bd[None, :], 5, mutant)
    return _shift(X, 5, mutant), _shift(Y, 5, mutant), X & 31, Y & 31


def canvas(src, rects_b, b, Hc, Wc, ys, xs, mutant=None, pinned=None):
    """(a): src uint8 [N,3,H,W]; rects_b int [4,8] or None -> (values int64 [3, ...], index of the rectangle or -1).
    `pinned` (the seam_first_rect mutant): take every tap from the rectangle of that index array, ignoring its own bounds"""
    N, _, H, W = src.shape
    ys, xs = np.asarray(ys), np.asarray(xs)
    if mutant == "replicate_border":
        ys, xs = np.clip(ys, 0, Hc - 1), np.clip(xs, 0, Wc - 1)
    if mutant == "flip_source_side_on":
        xs = Wc - 1 - xs
    out = np.zeros((3,) + ys.shape, np.int64)
    which = np.full(ys.shape, -1, np.int64)
    recs = [(0, 0, W, H, b, 0, 0, 0)] if rects_b is None else [tuple(int(t) for t in r) for r in rects_b]
    for k, (x1, y1, x2, y2, s, dx, dy, _pad) in enumerate(recs):
        cx1, cy1, cx2, cy2 = max(x1, 0), max(y1, 0), min(x2, Wc), min(y2, Hc)
        if cx2 <= cx1 or cy2 <= cy1:
            COUNTERS["rect_unused_slot"] += 1
            continue
        if (cx1, cy1, cx2, cy2) != (x1, y1, x2, y2):
            COUNTERS["rect_clipped_to_canvas"] += 1
        if not (0 <= s < N and cx1 - dx >= 0 and cx2 - dx <= W and cy1 - dy >= 0 and cy2 - dy <= H):
            COUNTERS["rect_skipped_outside_source"] += 1
            continue
        if pinned is None:
            inside = (xs >= cx1) & (xs < cx2) & (ys >= cy1) & (ys < cy2) & (which < 0)
        else:
            inside = (pinned == k) & (xs - dx >= 0) & (xs - dx < W) & (ys - dy >= 0) & (ys - dy < H)
        out[:, inside] = src[s][:, ys[inside] - dy, xs[inside] - dx]
        which[inside] = k
    return out, which


def rgb_to_hsv(r, g, b, mutant=None):
    """(c), first half: int64 arrays -> h (0..179), s, v"""
    sdiv, hdiv = div_tables()
    v = np.maximum(r, np.maximum(g, b))
    vmin = np.minimum(r, np.minimum(g, b))
    diff = v - vmin
    s = (diff * sdiv[v] + 2048) >> 12
    is_r, is_g = v == r, v == g
    if mutant == "g_before_r":
        h = np.where(is_g, b - r + 2 * diff, np.where(is_r, g - b, r - g + 4 * diff))
    else:
        h = np.where(is_r, g - b, np.where(is_g, b - r + 2 * diff, r - g + 4 * diff))
    COUNTERS["hsv_v_is_r"] += int(is_r.sum())
    COUNTERS["hsv_v_is_g"] += int((~is_r & is_g).sum())
    COUNTERS["hsv_v_is_b"] += int((~is_r & ~is_g).sum())
    h = (h * hdiv[diff] + 2048) >> 12
    COUNTERS["hsv_h_wrapped"] += int((h < 0).sum())
    if mutant == "no_h_plus_180":
        h = np.abs(h)                                            # any wrong hue will do; this one stays a valid index
    else:
        h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv_to_rgb(h, s, v, mutant=None):
    """(c), second half: int64 arrays (h <= 179) -> r, g, b int64"""
    assert int(h.max(initial=0)) <= 179, "sector = floor(h * 6/180) is 0..5 only for h <= 179"
    hf = h.astype(F) * (F(6.0) / F(180.0))
    sf = s.astype(F) * (F(1.0) / F(255.0))
    vf = v.astype(F) * (F(1.0) / F(255.0))
    sector = np.floor(hf)
    f = hf - sector
    sector = sector.astype(np.int64)
    assert sector.min(initial=0) >= 0 and sector.max(initial=0) <= 5
    one = F(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))])
    rows = np.array(SECTOR_TAB)
    if mutant == "sector_row_permuted":
        rows = rows[[0, 2, 1, 3, 4, 5]]
    grey = s == 0
    COUNTERS["hsv_grey"] += int(grey.sum())
    for k in range(6):
        COUNTERS["hsv_sector_%d" % k] += int(((sector == k) & ~grey).sum())
    idx = rows[sector]                                           # [..., 3]
    out = []
    for c in range(3):                                           # b, g, r
        x = np.take_along_axis(tab, idx[..., c][None], 0)[0]
        x = np.where(grey, vf, x)
        x = x * F(255.0)
        tie = x - np.floor(x) == F(0.5)
        COUNTERS["hsv_exact_tie"] += int(tie.sum())
        x = np.where(tie, np.floor(x) + F(1.0), np.rint(x)) if mutant == "round_half_away" else np.rint(x)
        out.append(np.clip(x, 0, 255).astype(np.int64))
    return out[2], out[1], out[0]


def _one(src, b, rects_b, Hc, Wc, m, Ho, Wo, lut, flip, mutant):
    """one output image of one stream: uint8 [3, Ho, Wo]"""
    shape = (Ho, Wo)
    if mutant == "swap_HoWo":
        Ho, Wo = Wo, Ho
    cm = "flip_source_side_on" if (mutant == "flip_source_side" and flip) else mutant
    if m is None:
        COUNTERS["warp_null"] += 1
        ys, xs = np.mgrid[0:Ho, 0:Wo]
        px, _ = canvas(src, rects_b, b, Hc, Wc, ys, xs, cm)
    else:
        COUNTERS["warp_matrix"] += 1
        sx, sy, fx, fy = warp_coords(m, Ho, Wo, mutant)
        COUNTERS["tap_negative"] += int(((sx < 0) | (sy < 0)).sum())
        COUNTERS["fraction_zero"] += int(((fx == 0) & (fy == 0)).sum())
        COUNTERS["fraction_nonzero"] += int(((fx != 0) | (fy != 0)).sum())
        taps, ids = [], []
        for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
            pin = ids[0] if (mutant == "seam_first_rect" and ids) else None
            t, w = canvas(src, rects_b, b, Hc, Wc, sy + oy, sx + ox, cm, pin)
            taps.append(t)
            ids.append(w)
        ids = np.stack(ids)
        COUNTERS["tap_outside_every_rect"] += int((ids < 0).sum())
        lo, hi = ids.min(0), ids.max(0)
        COUNTERS["quad_in_one_rect"] += int(((lo == hi) & (lo >= 0)).sum())
        COUNTERS["quad_partly_empty"] += int(((lo < 0) & (hi >= 0)).sum())
        lowest = np.where(ids >= 0, ids, 99).min(0)              # over the taps that hit a rectangle
        COUNTERS["quad_straddles_rects"] += int(((hi >= 0) & (lowest != hi)).sum())
        acc = (32 - fx) * (32 - fy) * taps[0] + fx * (32 - fy) * taps[1] + (32 - fx) * fy * taps[2] + fx * fy * taps[3]
        px = acc >> 10 if mutant == "truncate" else (acc + 512) >> 10
    r, g, bl = px[0], px[1], px[2]
    if lut is None:
        COUNTERS["jitter_none"] += 1
    else:
        h, s, v = rgb_to_hsv(r, g, bl, mutant)
        lut = np.asarray(lut).astype(np.int64)
        r, g, bl = hsv_to_rgb(lut[0][h], lut[1][s], lut[2][v], mutant)
    out = np.stack([r, g, bl]).astype(np.uint8)
    if flip is None:
        COUNTERS["flip_none"] += 1
    else:
        COUNTERS["flip_yes" if flip else "flip_no"] += 1
        if flip and mutant != "flip_source_side":
            out = out[:, :, ::-1]
    return np.ascontiguousarray(out).reshape((3,) + shape)


def augment(src_v, src_l, B=None, rects=None, canvas_size=None, minv=None, out_size=None, luts=None, flip=None, mutant=None):
    """dyk_augment_pairs: src uint8 [N,3,H,W] x 2; rects int [B,4,8] with canvas_size (Hc, Wc), or None; minv fp64 [B,6] (the
    INVERSE map, see invert()) or None; luts uint8 [B,3,256] or None; flip [B] or None -> (dst_v, dst_l) uint8 [B,3,Ho,Wo]"""
    src_v, src_l = np.asarray(src_v), np.asarray(src_l)
    assert src_v.dtype == np.uint8 and src_v.ndim == 4 and src_v.shape[1] == 3 and src_v.shape == src_l.shape
    N, _, H, W = src_v.shape
    B = N if B is None else B
    if rects is None:
        COUNTERS["rects_plain"] += 1
        assert B <= N
        Hc, Wc = H, W
    else:
        COUNTERS["rects_listed"] += 1
        Hc, Wc = canvas_size
    Ho, Wo = (Hc, Wc) if out_size is None else out_size
    if minv is None and (Ho, Wo) != (Hc, Wc):
        raise ValueError("no matrix: the output is the canvas")
    outs = []
    for stream, src in enumerate((src_v, src_l)):
        imgs = []
        for b in range(B):
            mb = b
            if mutant == "l_wrong_matrix" and stream == 1:
                mb = (b + 1) % B
            lb = 0 if mutant == "lut0_for_all" else b
            imgs.append(_one(src, b, None if rects is None else np.asarray(rects)[b], Hc, Wc, None if minv is None else minv[mb],
                             Ho, Wo, None if luts is None else luts[lb], None if flip is None else bool(flip[b]), mutant))
        outs.append(np.stack(imgs))
    return outs[0], outs[1]


def hsv_tables(r):
    """the three 256-entry tables of one image from its gains r = draw * [h_gain, s_gain, v_gain] + 1 (fp64 [3]), as
    reference kaist_dataset.py:498-501 forms them: int16 ramp times the gain in fp64; hue modulo 180, saturation and value
    clipped to 0..255; each truncated by the cast to uint8 -> uint8 [3,256]"""
    x = np.arange(0, 256, dtype=np.int16)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8),
                     np.clip(x * r[2], 0, 255).astype(np.uint8)])
