"""The yardstick of dyk_resize_pad_pairs (csrc/letterbox.hip): the rule of include/dyk_hip.h restated in plain numpy, slowly
and literally.  Every fp64 and fp32 operation of the rule is one numpy operation on arrays of that type, so nothing is
contracted; where the rule fixes an order (the taps of the weighted AREA form) the loops below run over the tap index in that
order and numpy only works across pixels, which are independent.  `area_pixel_scalar` is the same sum with scalar loops, for
the tests that hold the vectorised form to it.

It is derived from the classical OpenCV 8-bit resize, not measured against it: no cv2 runs where this project runs.

`mutant=` turns one rule into a plausible wrong one; tests/test_letterbox_reference.py shows that each is flagged by a named
case of tests/letterbox_cases.py:
  shift22             vertical pass as (b0*D0 + b1*D1 + 2^21) >> 22
  scale_src_over_dst  scale = n_src / n_dst instead of 1 / (n_dst / n_src)
  no_edge_exception   right edge: taps clamped and coefficients kept, instead of sx = w-1, fx = 0 and D = S * 2048
  fy_reset_top        rows with sy < 0 reset to sy = 0, fy = 0 as the columns are
  half_away           coefficients rounded half away from zero
  area2_float         2 x 2 AREA as rn(sum * 0.25f)
  area_fma            weighted AREA with fused multiply-adds
  no_eps              the two 1e-3 tests of the weighted AREA taps replaced by > 0
  pad_off_by_one      content one row lower
  no_channel_reverse  interleaved layout without the channel reversal
  swap_top_left       top and left exchanged
  linear2x_not_switched  LINEAR at exactly 2 x stays LINEAR
"""
import math

import numpy as np

LINEAR, AREA = 0, 1
MAX_SIZE = 16384
MUTANTS = ("shift22", "scale_src_over_dst", "no_edge_exception", "fy_reset_top", "half_away", "area2_float", "area_fma", "no_eps",
           "pad_off_by_one", "no_channel_reverse", "swap_top_left", "linear2x_not_switched")

f32 = np.float32


def axis_scale(n_src, n_dst, mutant=None):
    """scale of one axis: two roundings, inv = n_dst / n_src, then 1 / inv"""
    if mutant == "scale_src_over_dst":
        return float(n_src) / float(n_dst)
    inv = float(n_dst) / float(n_src)
    return 1.0 / inv


def _rn_coef(x, mutant):
    """rn of a fp32 coefficient array -> int32"""
    if mutant == "half_away":
        return np.floor(x.astype(np.float64) + 0.5).astype(np.int32)
    return np.rint(x).astype(np.int32)                       # half to even


def linear_coeffs(n_src, n_dst, edge_reset, mutant=None):
    """-> (s int32 [n_dst] before any clamping of taps, c0, c1 int32 [n_dst]).  edge_reset: the column form (both resets);
    without it the row form (coefficients as computed, the caller clamps the two tap rows)"""
    scale = axis_scale(n_src, n_dst, mutant)
    d = np.arange(n_dst, dtype=np.float64)
    t = d + 0.5
    t = t * scale
    t = t - 0.5
    f = t.astype(f32)                                        # cast once
    s = np.floor(f)
    f = f - s                                                # fp32
    s = s.astype(np.int32)
    if edge_reset or mutant == "fy_reset_top":
        low = s < 0
        s = np.where(low, 0, s).astype(np.int32)
        f = np.where(low, f32(0), f).astype(f32)
    if edge_reset and mutant != "no_edge_exception":
        high = s >= n_src - 1
        s = np.where(high, n_src - 1, s).astype(np.int32)
        f = np.where(high, f32(0), f).astype(f32)
    c0 = _rn_coef((f32(1) - f) * f32(2048), mutant)
    c1 = _rn_coef(f * f32(2048), mutant)
    return s, c0, c1


def resize_linear(S, nh, nw, mutant=None):
    """S uint8 [..., h, w] -> uint8 [..., nh, nw]"""
    h, w = S.shape[-2:]
    sx, a0, a1 = linear_coeffs(w, nw, True, mutant)
    sy, b0, b1 = linear_coeffs(h, nh, False, mutant)
    Si = S.astype(np.int32)
    if mutant == "no_edge_exception":
        x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
        D = Si[..., :, x0] * a0 + Si[..., :, x1] * a1
    else:
        edge = sx + 1 >= w
        x1 = np.where(edge, sx, sx + 1)
        D = np.where(edge, Si[..., :, sx] * 2048, Si[..., :, sx] * a0 + Si[..., :, x1] * a1)
    D0 = D[..., np.clip(sy, 0, h - 1), :]
    D1 = D[..., np.clip(sy + 1, 0, h - 1), :]
    b0, b1 = b0[:, None], b1[:, None]
    if mutant == "shift22":
        out = (b0.astype(np.int64) * D0 + b1.astype(np.int64) * D1 + (1 << 21)) >> 22
    else:
        out = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def area_taps(n_src, n_dst, mutant=None):
    """the taps of the weighted AREA form of one axis, in the rule's order -> a list per destination index of (s, fp32 weight)"""
    scale = axis_scale(n_src, n_dst, mutant)
    eps = 0.0 if mutant == "no_eps" else 1e-3
    out = []
    for d in range(n_dst):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, n_src - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), n_src - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > eps:
            taps.append((s1 - 1, f32((s1 - f1) / cell)))
        for s in range(s1, s2):
            taps.append((s, f32(1.0 / cell)))
        if f2 - s2 > eps:
            taps.append((s2, f32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(taps)
    return out


def _tap_arrays(taps):
    """list of tap lists -> (idx int [K, n], weight fp32 [K, n], valid bool [K, n]), K the longest list"""
    K = max(len(t) for t in taps)
    idx = np.zeros((K, len(taps)), np.int64)
    wt = np.zeros((K, len(taps)), f32)
    ok = np.zeros((K, len(taps)), bool)
    for d, t in enumerate(taps):
        for k, (s, a) in enumerate(t):
            idx[k, d], wt[k, d], ok[k, d] = s, a, True
    return idx, wt, ok


def _sat_rn(acc):
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def _mad(a, b, c, mutant):
    """a * b + c in fp32: two roundings (one with the area_fma mutant)"""
    if mutant == "area_fma":
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    return (a * b).astype(f32) + c


def resize_area(S, nh, nw, mutant=None):
    """S uint8 [..., h, w] -> uint8 [..., nh, nw]; nh <= h and nw <= w"""
    h, w = S.shape[-2:]
    assert nh <= h and nw <= w
    if w % nw == 0 and h % nh == 0:
        kx, ky = w // nw, h // nh
        s = S.astype(np.int32).reshape(S.shape[:-2] + (nh, ky, nw, kx)).sum(axis=(-3, -1), dtype=np.int32)
        if kx == 2 and ky == 2 and mutant != "area2_float":
            return ((s + 2) >> 2).astype(np.uint8)
        return _sat_rn(s.astype(f32) * (f32(1) / f32(kx * ky)))
    xi, xw, xok = _tap_arrays(area_taps(w, nw, mutant))
    yi, yw, yok = _tap_arrays(area_taps(h, nh, mutant))
    Sf = S.astype(f32)
    acc = np.zeros(S.shape[:-2] + (nh, nw), f32)
    for ky in range(yi.shape[0]):                            # row taps in order
        rows = Sf[..., yi[ky], :]                            # [..., nh, w]
        buf = np.zeros_like(acc)
        for kx in range(xi.shape[0]):                        # column taps in order
            buf = np.where(xok[kx], _mad(rows[..., xi[kx]], xw[kx], buf, mutant), buf)
        beta = yw[ky][:, None]
        if ky == 0:
            step = (beta * buf).astype(f32)
        else:
            step = _mad(beta, buf, acc, mutant)
        acc = np.where(yok[ky][:, None], step, acc)
    return _sat_rn(acc)


def area_pixel_scalar(S, ytaps, xtaps):
    """one output pixel of the weighted AREA form with scalar loops: S uint8 [h, w], the taps of its row and column"""
    acc = None
    for sy, beta in ytaps:
        buf = f32(0)
        for sx, alpha in xtaps:
            buf = f32(buf + f32(f32(S[sy, sx]) * alpha))
        acc = f32(beta * buf) if acc is None else f32(acc + f32(beta * buf))
    return int(min(max(np.rint(acc), 0), 255))


def resize(S, nh, nw, interp, mutant=None):
    """S uint8 [..., h, w] planes -> uint8 [..., nh, nw]"""
    h, w = S.shape[-2:]
    if nh == h and nw == w:
        return S.copy()
    if interp == LINEAR and w == 2 * nw and h == 2 * nh and mutant != "linear2x_not_switched":
        interp = AREA
    if interp == AREA:
        return resize_area(S, nh, nw, mutant)
    return resize_linear(S, nh, nw, mutant)


def check(shape, geom, out_size):
    """what the entry refuses, for one image: shape (h, w), geom (nh, nw, top, left, interp) -> None, or the reason"""
    h, w = shape
    nh, nw, top, left, interp = geom
    Ho, Wo = out_size
    if min(h, w, nh, nw, Ho, Wo) < 1:
        return "a size below 1"
    if max(h, w, nh, nw, Ho, Wo) > MAX_SIZE:
        return "a size above %d" % MAX_SIZE
    if interp not in (LINEAR, AREA):
        return "interp"
    if top < 0 or left < 0 or top + nh > Ho or left + nw > Wo:
        return "the content rectangle does not lie inside the output"
    if interp == AREA and (nw > w or nh > h):
        return "AREA does not enlarge"
    return None


def planes_of(img, layout):
    """an image in `layout` ("chw" [3,h,w] / "hwc_bgr" [h,w,3]) -> its OUTPUT planes [3,h,w]"""
    if layout == "chw":
        return img
    return np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1))


def resize_pad(v_list, l_list, geom, out_size, layout="chw", color=(0, 0, 0), mutant=None):
    """the whole entry: lists of B source images per stream, geom [B] of (nh, nw, top, left, interp) -> (ov, ol) uint8 [B,3,Ho,Wo]"""
    Ho, Wo = out_size
    B = len(geom)
    outs = []
    for srcs in (v_list, l_list):
        out = np.empty((B, 3, Ho, Wo), np.uint8)
        out[:] = np.asarray(color, np.uint8)[None, :, None, None]
        for b in range(B):
            img = np.asarray(srcs[b])
            nh, nw, top, left, interp = (int(t) for t in geom[b])
            why = check(img.shape[1:] if layout == "chw" else img.shape[:2], (nh, nw, top, left, interp), out_size)
            if why:
                raise ValueError(why)
            P = planes_of(img, layout)
            if layout != "chw" and mutant == "no_channel_reverse":
                P = P[::-1]
            if mutant == "swap_top_left":
                top, left = left, top
            if mutant == "pad_off_by_one":
                top += 1
            R = resize(P, nh, nw, interp, mutant)
            y0, x0 = max(top, 0), max(left, 0)                   # (only a mutant can leave the output; it is cut there)
            y1, x1 = min(top + nh, Ho), min(left + nw, Wo)
            if y1 > y0 and x1 > x0:
                out[b, :, y0:y1, x0:x1] = R[:, y0 - top:y1 - top, x0 - left:x1 - left]
        outs.append(out)
    return outs[0], outs[1]


def letterbox_geometry(shape, new_shape=(416, 416), auto=True, scale_fill=False, scale_up=True):
    """the host half of the reference's letterbox, restated: shape (h, w) -> (ratio, (dw, dh), (nh, nw), (top, bottom, left, right))"""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scale_up:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = dw % 64, dh % 64
    elif scale_fill:
        dw, dh = 0, 0
        new_unpad = new_shape
        ratio = new_shape[0] / shape[1], new_shape[1] / shape[0]
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return ratio, (dw, dh), (int(new_unpad[1]), int(new_unpad[0])), (top, bottom, left, right)
