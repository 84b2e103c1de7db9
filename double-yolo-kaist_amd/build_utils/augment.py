"""The random training augmentation of the reference's default loader (LoadKaistImagesAndLabels(augment=True, rect=False),
reference build_utils/kaist_dataset.py) with every pixel made on the MI355X: the four-image mosaic (load_quadra_images,
:213-286), random_affine (:408-479), augment_hsv (:482-506) and the left-right flip of __getitem__ (:362-369).  One launch of
dyk_augment_pairs (csrc/augment.hip; the rule is in include/dyk_hip.h) makes both streams of a whole batch.

Images are uint8 device tensors in the loader's planar RGB layout, [3,H,W] or [B,3,H,W]; labels stay on the host.  The random
draws and the label arithmetic are host Python / numpy and follow the reference draw for draw, so seeding `random` and
`np.random` reproduces the decisions of a single-worker reference loader.  Nothing here synchronises the device: the
matrices, rectangles, tables and flip flags of a batch go up in one small copy.  Importing this module needs no cv2.

The pixel rule is the classical OpenCV 8-bit path -- warpAffine(INTER_LINEAR, border 0), cvtColor BGR2HSV, cv2.LUT,
cvtColor HSV2BGR -- as this project's own rule; agreement with cv2 itself is derived, not measured (none is installed where
this project runs, and newer OpenCV releases changed their warp kernels).

Kept on purpose, because a model trained with the reference saw them:
  * random_affine scales the x translation by the image HEIGHT and the y translation by its WIDTH (kaist_dataset.py:435-436);
  * the mosaic's third tile takes its source columns up to max(xr, w) (:246); the slice clips that to w, so only the canvas
    rectangle and the offsets matter, and those are what is kept.
Different from the reference, and you must know it:
  * mosaic() and augment_batch(mosaic=True) draw the three companions of an image from the SAME BATCH, not from the whole data
    set (the other images are not on the device).  What that costs in AP is not measured;
  * augment_batch takes the collate function's normalised xywh targets, so its labels go xywh -> pixel xyxy -> transform ->
    xywh: one rounding more than the reference, which never normalises in between.  Label arithmetic is fp64, cast back once.
"""
import math
import random

import numpy as np
import torch

from build_utils.utils import xyxy2xywh

_NO_HYP = {"degrees": 0, "translate": 0, "scale": 0, "shear": 0, "hsv_h": 0, "hsv_s": 0, "hsv_v": 0}


def _draw_matrix(rows, cols, degrees, translate, scale, shear, border):
    """The six random.uniform draws of random_affine in the reference's order (angle, scale, T[0,2], T[1,2], S[0,1], S[1,0];
    kaist_dataset.py:428-444) -> (M = S @ T @ R fp64 [3,3], the drawn scale).  cv2.getRotationMatrix2D about the centre
    (cols / 2, rows / 2) is written out: alpha = s cos a, beta = s sin a,
    [[alpha, beta, (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]]."""
    a = random.uniform(-degrees, degrees)
    s = random.uniform(1 - scale, 1 + scale)
    cx, cy = cols / 2, rows / 2
    rad = a * math.pi / 180
    alpha, beta = math.cos(rad) * s, math.sin(rad) * s
    R = np.eye(3)
    R[0] = [alpha, beta, (1 - alpha) * cx - beta * cy]
    R[1] = [-beta, alpha, beta * cx + (1 - alpha) * cy]
    T = np.eye(3)
    T[0, 2] = random.uniform(-translate, translate) * rows + border      # the reference's quirk: x moves by the HEIGHT ...
    T[1, 2] = random.uniform(-translate, translate) * cols + border      # ... and y by the WIDTH (:435-436); kept
    S = np.eye(3)
    S[0, 1] = math.tan(random.uniform(-shear, shear) * math.pi / 180)
    S[1, 0] = math.tan(random.uniform(-shear, shear) * math.pi / 180)
    return S @ T @ R, s


def _warp_labels(labels, M, s, width, height):
    """labels fp64 [n,5] (class, xyxy in pixels) through M (kaist_dataset.py:452-477): the four corners of every box are
    mapped, the new box is their bounding box clipped to the output, and a box is kept when it is more than 4 pixels on both
    sides, keeps more than 0.2 of its area (scaled by s) and is less than 10 : 1 -> the kept labels, a new array"""
    n = labels.shape[0]
    if n == 0:
        return labels
    corners = np.ones((n * 4, 3))
    corners[:, :2] = labels[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)          # x1y1, x2y2, x1y2, x2y1
    corners = (corners @ M.T)[:, :2].reshape(n, 8)
    xs, ys = corners[:, [0, 2, 4, 6]], corners[:, [1, 3, 5, 7]]
    box = np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), 1)
    box[:, [0, 2]] = box[:, [0, 2]].clip(0, width)
    box[:, [1, 3]] = box[:, [1, 3]].clip(0, height)
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    area0 = (labels[:, 3] - labels[:, 1]) * (labels[:, 4] - labels[:, 2])
    aspect = np.maximum(w / (h + 1e-16), h / (w + 1e-16))
    keep = (w > 4) & (h > 4) & (w * h / (area0 * s + 1e-16) > 0.2) & (aspect < 10)
    out = labels[keep]
    out[:, 1:5] = box[keep]
    return out


def _labels_in(labels):
    """-> (fp64 numpy [n,5] copy, a function that gives the result the type it came in)"""
    if isinstance(labels, torch.Tensor):
        dt = labels.dtype
        return labels.detach().cpu().numpy().astype(np.float64).reshape(-1, 5), lambda a: torch.from_numpy(a).to(dt)
    a = np.asarray(labels)
    dt = a.dtype if a.dtype.kind == "f" else np.float64
    return a.astype(np.float64).reshape(-1, 5), lambda a: a.astype(dt)


def _pair(v_img, l_img, what):
    if not isinstance(v_img, torch.Tensor) or not isinstance(l_img, torch.Tensor) or v_img.shape != l_img.shape or v_img.dim() not in (3, 4):
        raise ValueError("%s: two uint8 device tensors of one shape, [3,H,W] or [B,3,H,W]" % what)
    return (v_img[None], l_img[None], True) if v_img.dim() == 3 else (v_img, l_img, False)


def random_affine(v_img, l_img, labels=(), degrees=10, translate=0.1, scale=0.1, shear=0.1, border=0):
    """The reference's random_affine (kaist_dataset.py:408-479) on a device pair [3,H,W] (or a batch [B,3,H,W] under ONE
    matrix): rotation and scale about the centre, translation, shear, into an output of (H + 2 border) x (W + 2 border) ->
    (v, l, labels).  `labels` [n,5] (class, xyxy in pixels; numpy or CPU tensor) are transformed and filtered as the reference
    does and come back in the type they came in.  With border == 0 and an identity matrix the images are returned as they are."""
    from dyk.functional import augment_pairs
    v4, l4, single = _pair(v_img, l_img, "random_affine")
    H, W = int(v4.shape[2]), int(v4.shape[3])
    height, width = H + border * 2, W + border * 2
    M, s = _draw_matrix(H, W, degrees, translate, scale, shear, border)
    if border != 0 or (M != np.eye(3)).any():
        B = int(v4.shape[0])
        v4, l4 = augment_pairs(v4, l4, matrices=np.repeat(M[None, :2], B, 0), out_size=(height, width))
        v_img, l_img = (v4[0], l4[0]) if single else (v4, l4)
    if len(labels) > 0:
        lab, back = _labels_in(labels)
        labels = back(_warp_labels(lab, M, s, width, height))
    return v_img, l_img, labels


def _hsv_tables(h_gain, s_gain, v_gain):
    """one np.random.uniform(-1, 1, 3) draw -> the hue / saturation / value tables uint8 [3,256] (kaist_dataset.py:493-501):
    an int16 ramp times the gain in fp64, hue modulo 180, the others clipped to 0..255, truncated by the cast"""
    r = np.random.uniform(-1, 1, 3) * [h_gain, s_gain, v_gain] + 1
    x = np.arange(0, 256, dtype=np.int16)
    return np.stack((((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8),
                     np.clip(x * r[2], 0, 255).astype(np.uint8)))


def augment_hsv(v_img, l_img, h_gain=0.5, s_gain=0.5, v_gain=0.5):
    """The reference's augment_hsv (kaist_dataset.py:482-506): one draw of three gains, both images through RGB -> HSV ->
    tables -> RGB IN PLACE; returns None.  A batch [B,3,H,W] gets the one draw for all its images."""
    from dyk.functional import augment_pairs
    v4, l4, _ = _pair(v_img, l_img, "augment_hsv")
    tables = _hsv_tables(h_gain, s_gain, v_gain)
    augment_pairs(v4, l4, luts=np.repeat(tables[None], int(v4.shape[0]), 0), out=(v4, l4))


def _tile_span(centre, n, limit, before):
    """One axis of a mosaic tile of n pixels that touches `centre` on a canvas of `limit` pixels: a tile before the centre ends
    there and is cut at 0 (it keeps its far end), one after it starts there and is cut at `limit` (it keeps its near end)
    -> (canvas lo, canvas hi, offset with source = canvas - offset); the offset is the reference's padw / padh"""
    if before:
        return max(centre - n, 0), centre, centre - n
    return centre, min(centre + n, limit), centre


def _xywh_to_pixels(x, w, h, padw=0, padh=0):
    """labels [n,5] (class, xywh normalised to a w x h image) -> a copy with xyxy in pixels, moved by (padw, padh); the
    arithmetic of kaist_dataset.py:261-264, size * (centre -/+ extent / 2) + pad, both corners at once"""
    out = x[:, :5].copy()
    size, pad = np.array([w, h], np.float64), np.array([padw, padh], np.float64)
    out[:, 1:3] = size * (x[:, 1:3] - x[:, 3:5] / 2) + pad
    out[:, 3:5] = size * (x[:, 1:3] + x[:, 3:5] / 2) + pad
    return out


def _draw_mosaic(index, B, s, sizes, labels_per_image):
    """The draws and the placement of load_quadra_images (kaist_dataset.py:224-272) for output sample `index` of a batch of B:
    the centre (xr, yr) by two random.uniform(0.5 s, 1.5 s) truncated, three companions by random.randint(0, B - 1); tile i
    goes above-left, above-right, below-left, below-right of the centre on the 2s x 2s canvas -> (rects int32 [4,8] with
    dx = padw, dy = padh, labels fp64 [n,5] in canvas pixels, clipped to the canvas).  sizes[j] = (h, w) of image j;
    labels_per_image[j] = [n,5] (class, xywh normalised)."""
    centre = [int(random.uniform(s * 0.5, s * 1.5)) for _ in range(2)]                # (xr, yr)
    members = [index] + [random.randint(0, B - 1) for _ in range(3)]
    rects = np.zeros((4, 8), np.int32)
    labels4 = []
    for slot, j in enumerate(members):                           # above-left, above-right, below-left, below-right
        (x_lo, x_hi, dx), (y_lo, y_hi, dy) = (_tile_span(c, n, 2 * s, before)
                                              for c, n, before in ((centre[0], sizes[j][1], slot % 2 == 0), (centre[1], sizes[j][0], slot < 2)))
        rects[slot] = (x_lo, y_lo, x_hi, y_hi, j, dx, dy, 0)
        labels4.append(_xywh_to_pixels(np.asarray(labels_per_image[j], np.float64).reshape(-1, 5), sizes[j][1], sizes[j][0], dx, dy))
    labels4 = np.concatenate(labels4, 0)
    np.clip(labels4[:, 1:], 0, 2 * s, out=labels4[:, 1:])
    return rects, labels4


def mosaic(v_imgs, l_imgs, labels_per_image, index, img_size=None, hyp=None):
    """load_quadra_images (kaist_dataset.py:213-286) for ONE output sample drawn from a device batch [B,3,h,w]: image `index`
    and three companions drawn FROM THE SAME BATCH (not from the whole data set, as the reference does) around a random centre
    of a 2s x 2s canvas, then random_affine(border=-s // 2) with hyp's degrees / translate / scale / shear (all 0 without
    hyp) -- canvas and warp in the one launch; the canvas is never materialised.  s = img_size (default max(h, w)).
    labels_per_image[j]: [n,5] (class, xywh normalised) of image j -> (v, l, labels): [3,S,S] images with S = 2s + 2(-s // 2),
    labels fp64 numpy [m,5] (class, xyxy in pixels of the output)."""
    from dyk.functional import augment_pairs
    if not isinstance(v_imgs, torch.Tensor) or v_imgs.dim() != 4 or v_imgs.shape != l_imgs.shape:
        raise ValueError("mosaic: two [B,3,h,w] batches of one shape")
    B, h, w = int(v_imgs.shape[0]), int(v_imgs.shape[2]), int(v_imgs.shape[3])
    if len(labels_per_image) != B or not 0 <= index < B:
        raise ValueError("mosaic: labels for each of the %d images and an index among them" % B)
    hyp = _NO_HYP if hyp is None else hyp
    s = max(h, w) if img_size is None else int(img_size)
    rects, labels4 = _draw_mosaic(index, B, s, [(h, w)] * B, labels_per_image)
    border = -s // 2
    side = 2 * s + 2 * border
    M, sc = _draw_matrix(2 * s, 2 * s, hyp["degrees"], hyp["translate"], hyp["scale"], hyp["shear"], border)
    ov, ol = augment_pairs(v_imgs, l_imgs, matrices=M[None, :2], rects=rects[None], canvas=(2 * s, 2 * s), out_size=(side, side))
    return ov[0], ol[0], _warp_labels(labels4, M, sc, side, side)


def augment_batch(v_imgs, l_imgs, targets, hyp, mosaic=False, flip=True, img_size=None):
    """What the training loop calls after `.to(device)` on a batch the loader made with augment=False: device uint8 [B,3,H,W]
    batches and the collate function's host targets [n,6] (image, class, xywh normalised) -> (v, l, targets) of the augmented
    batch, the targets in the same form and type.  ONE launch.  Per image, in batch order, the draws are those of one
    __getitem__ of the reference: with `mosaic` the centre and the three companions (from this batch), the six draws of
    random_affine (border = -s // 2 on the 2s x 2s canvas with mosaic, s = img_size or max(H, W); 0 on the image without),
    one np.random.uniform(-1, 1, 3) for the HSV tables (hyp's hsv_h / hsv_s / hsv_v), and with `flip` one random.random()
    for the left-right flip.  The output is [B,3,S,S] with mosaic (S = 2s + 2(-s // 2)), [B,3,H,W] without."""
    from dyk.functional import augment_pairs
    if not isinstance(v_imgs, torch.Tensor) or v_imgs.dim() != 4 or v_imgs.shape != l_imgs.shape:
        raise ValueError("augment_batch: two [B,3,H,W] batches of one shape")
    B, H, W = int(v_imgs.shape[0]), int(v_imgs.shape[2]), int(v_imgs.shape[3])
    is_tensor = isinstance(targets, torch.Tensor)
    t = (targets.detach().cpu().numpy() if is_tensor else np.asarray(targets)).astype(np.float64).reshape(-1, 6)
    per_image = [t[t[:, 0] == b, 1:] for b in range(B)]
    s = max(H, W) if img_size is None else int(img_size)
    border = -s // 2 if mosaic else 0
    Ho, Wo = (2 * s + 2 * border,) * 2 if mosaic else (H, W)
    mats, luts, flips, out_t = np.zeros((B, 2, 3)), np.zeros((B, 3, 256), np.uint8), np.zeros(B, np.uint8), []
    rects = np.zeros((B, 4, 8), np.int32) if mosaic else None
    for b in range(B):
        if mosaic:
            rects[b], lab = _draw_mosaic(b, B, s, [(H, W)] * B, per_image)
            M, sc = _draw_matrix(2 * s, 2 * s, hyp["degrees"], hyp["translate"], hyp["scale"], hyp["shear"], border)
        else:
            lab = _xywh_to_pixels(per_image[b], W, H)
            M, sc = _draw_matrix(H, W, hyp["degrees"], hyp["translate"], hyp["scale"], hyp["shear"], 0)
        mats[b] = M[:2]
        lab = _warp_labels(lab, M, sc, Wo, Ho)
        luts[b] = _hsv_tables(hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"])
        if lab.shape[0]:
            lab[:, 1:5] = xyxy2xywh(lab[:, 1:5])
            lab[:, [2, 4]] /= Ho
            lab[:, [1, 3]] /= Wo
        if flip and random.random() < 0.5:
            flips[b] = 1
            if lab.shape[0]:
                lab[:, 1] = 1 - lab[:, 1]
        out_t.append(np.concatenate((np.full((lab.shape[0], 1), float(b)), lab), 1))
    plain = not mosaic and all((mats[b] == np.eye(3)[:2]).all() for b in range(B))      # as the reference skips the warp
    ov, ol = augment_pairs(v_imgs, l_imgs, matrices=None if plain else mats, rects=rects, canvas=(2 * s, 2 * s) if mosaic else None,
                           out_size=(Ho, Wo), luts=luts, flip=flips if flip else None)
    out_t = np.concatenate(out_t, 0) if out_t else np.zeros((0, 6))
    if is_tensor:
        return ov, ol, torch.from_numpy(out_t).to(targets.dtype)
    return ov, ol, out_t.astype(np.asarray(targets).dtype if np.asarray(targets).dtype.kind == "f" else np.float64)
