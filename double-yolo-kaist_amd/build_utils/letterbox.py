"""The resize and letterbox of the reference's loader with every pixel made on the MI355X: the cv2.resize at the end of
LoadKaistImagesAndLabels.load_image (reference build_utils/kaist_dataset.py:204-208), letterbox (build_utils/img_utils.py:5-53,
called from kaist_dataset.py:293-294 and detect.py:33-34), the label arithmetic of load_normal_images (:303-306) and the
BGR HWC -> RGB CHW of __getitem__ (:378-379).  One launch of dyk_resize_pad_pairs (csrc/letterbox.hip; the rule is in
include/dyk_hip.h) makes both streams of a whole batch, so a loader worker only has to decode the files.

This module is NOT build_utils.img_utils: that name keeps resolving to the reference, whose unchanged loader calls it with
numpy arrays inside its workers.  Images here are uint8 device tensors, planar RGB [3,h,w] (layout "chw") or cv2.imread's
[h,w,3] BGR (layout "hwc_bgr"); the geometry and the labels stay on the host and are computed exactly as the reference
computes them (Python `round`, np.mod under `auto`, int(round(d -/+ 0.1)) for the two sides).  Nothing synchronises the device.
Importing this module needs no cv2.

The pixel rule is the classical OpenCV 8-bit resize (INTER_LINEAR, INTER_AREA) as this project's own rule; agreement with cv2
itself is derived, not measured (none is installed where this project runs; OpenCV builds with IPP or newer SIMD paths may
differ).  Limits: uint8, sizes up to 16384, AREA only shrinks (the reference never asks for more: kaist_dataset.py:206), no
INTER_CUBIC / LANCZOS / NEAREST.

Kept on purpose, because the reference does it: under `scale_fill` (and not `auto`) `ratio` is (new_shape[0] / width,
new_shape[1] / height) -- the HEIGHT of new_shape over the image width and its WIDTH over the image height -- and
`new_unpad = new_shape` is handed to the resize as (width, height), so a non-square new_shape = (H, W) yields an image of W rows
and H columns (img_utils.py:38-41).
"""
import numpy as np
import torch

from dyk import functional as F

LINEAR, AREA = F.RESIZE_LINEAR, F.RESIZE_AREA


def _geometry(shape, new_shape, auto, scale_fill, scale_up):
    """img_utils.py:22-50 on the host: shape (h, w) -> (ratio, (dw, dh), (nh, nw), (top, bottom, left, right))"""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scale_up:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, 64), np.mod(dh, 64)
    elif scale_fill:
        dw, dh = 0, 0
        new_unpad = new_shape                                    # the quirk: (h, w) handed on as (width, height)
        ratio = new_shape[0] / shape[1], new_shape[1] / shape[0]
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return ratio, (dw, dh), (int(new_unpad[1]), int(new_unpad[0])), (top, bottom, left, right)


def _hw(img, layout):
    if not isinstance(img, torch.Tensor) or img.dim() != 3:
        raise TypeError("a uint8 device image %s, got %s" % ("[3,h,w]" if layout == "chw" else "[h,w,3]",
                                                             tuple(img.shape) if isinstance(img, torch.Tensor) else type(img).__name__))
    return (int(img.shape[1]), int(img.shape[2])) if layout == "chw" else (int(img.shape[0]), int(img.shape[1]))


def letterbox_pair(v_img, l_img, new_shape=(416, 416), color=(0, 0, 0), auto=True, scale_fill=False, scale_up=True):
    """letterbox of both streams of one pair in one launch -> (v, l, ratio, (dw, dh)); v_img, l_img uint8 device [3,h,w] of one
    size.  See letterbox."""
    shape = _hw(v_img, "chw")
    ratio, pad, (nh, nw), (top, bottom, left, right) = _geometry(shape, new_shape, auto, scale_fill, scale_up)
    ov, ol = F.resize_pad_pairs([v_img], [l_img], [(nh, nw, top, left, LINEAR)], (nh + top + bottom, nw + left + right), color=color)
    return ov[0], ol[0], ratio, pad


def letterbox(img, new_shape=(416, 416), color=(0, 0, 0), auto=True, scale_fill=False, scale_up=True):
    """The reference's letterbox (img_utils.py:5-53: name, signature, return (img, ratio, (dw, dh))) on a uint8 device image
    [3,h,w]: scaled by r = min(new_shape / shape) (at most 1 without `scale_up`) with INTER_LINEAR, then padded with `color` to
    new_shape -- under `auto` only to the next multiple of 64 -- with int(round(d - 0.1)) on the top / left and
    int(round(d + 0.1)) on the bottom / right.  `scale_fill` (without `auto`) stretches instead, with the reference's quirks
    (module text).  For a pair use letterbox_pair: this call runs the pair entry on the one image twice."""
    v, _, ratio, pad = letterbox_pair(img, img, new_shape, color, auto, scale_fill, scale_up)
    return v, ratio, pad


def _load_size(h0, w0, img_size, augment):
    """the tail of load_image on the host: -> ((h, w), interp) of the resized image; (h0, w0) itself when r == 1"""
    r = img_size / max(h0, w0)
    if r == 1:
        return (h0, w0), LINEAR
    return (int(h0 * r), int(w0 * r)), (AREA if r < 1 and not augment else LINEAR)


def load_resize(v_img, l_img, img_size, augment):
    """The tail of load_image (kaist_dataset.py:204-211) on a pair of uint8 device images [3,h0,w0]: r = img_size / max(h0, w0),
    size (int(w0 * r), int(h0 * r)), INTER_AREA when r < 1 and not augment, else INTER_LINEAR; the images themselves when
    r == 1.  -> (v, l, (h0, w0), (h, w))"""
    h0, w0 = _hw(v_img, "chw")
    (h, w), interp = _load_size(h0, w0, img_size, augment)
    if (h, w) == (h0, w0):
        return v_img, l_img, (h0, w0), (h0, w0)
    ov, ol = F.resize_pad_pairs([v_img], [l_img], [(h, w, 0, 0, interp)], (h, w))
    return ov[0], ol[0], (h0, w0), (h, w)


def letterbox_labels(x, ratio, pad, w, h):
    """kaist_dataset.py:303-306 on the host: labels x [n,5] (class, normalised xywh of the w x h image before the letterbox)
    -> a new array (class, xyxy in pixels of the letterboxed image)"""
    x = np.asarray(x)
    labels = x.copy()
    if x.size > 0:
        labels[:, 1] = ratio[0] * w * (x[:, 1] - x[:, 3] / 2) + pad[0]
        labels[:, 2] = ratio[1] * h * (x[:, 2] - x[:, 4] / 2) + pad[1]
        labels[:, 3] = ratio[0] * w * (x[:, 1] + x[:, 3] / 2) + pad[0]
        labels[:, 4] = ratio[1] * h * (x[:, 2] + x[:, 4] / 2) + pad[1]
    return labels


def letterbox_batch(v_imgs, l_imgs, new_shape, img_size=None, augment=False, auto=False, scale_up=None, color=(0, 0, 0), layout="chw",
                    labels=None):
    """What load_normal_images does per sample (kaist_dataset.py:288-306), for a whole batch of raw frames on the device:
    the load_image resize to `img_size` (skipped when img_size is None) and the letterbox to `new_shape`, `scale_up` defaulting
    to `augment` as the loader passes it.  v_imgs, l_imgs: a batch tensor or lists of per-image tensors of different sizes;
    layout "chw" (planar RGB) or "hwc_bgr" (cv2.imread's array as it is).  labels: per image [n,5] (class, normalised xywh) or
    None.  -> (v [B,3,Ho,Wo], l, shapes, labels) with shapes[b] = ((h0, w0), ((h / h0, w / w0), pad)) as the loader emits it
    for scale_coords, and labels[b] (class, xyxy in pixels) through letterbox_labels.
    ONE launch whenever, for every image, at most one of the two steps changes the size (always so for KAIST frames: 512 x 640
    to img_size 512 and new_shape 512 only pads in the second step).  Otherwise every image goes through its first step into a
    planar intermediate (one launch per distinct intermediate size) and one final launch makes the letterbox from those, so the
    result is the reference's two successive resizes in every case.  ValueError when the images do not end at one output size."""
    vs = list(v_imgs.unbind(0)) if isinstance(v_imgs, torch.Tensor) else list(v_imgs)
    ls = list(l_imgs.unbind(0)) if isinstance(l_imgs, torch.Tensor) else list(l_imgs)
    if len(vs) < 1 or len(vs) != len(ls):
        raise ValueError("letterbox_batch: %d visible and %d LWIR images" % (len(vs), len(ls)))
    if layout not in ("chw", "hwc_bgr"):
        raise ValueError("letterbox_batch: layout is 'chw' or 'hwc_bgr', got %r" % (layout,))
    scale_up = augment if scale_up is None else scale_up
    plan, shapes, out_size = [], [], None
    for b, v in enumerate(vs):
        h0, w0 = _hw(v, layout)
        (h, w), interp1 = ((h0, w0), LINEAR) if img_size is None else _load_size(h0, w0, img_size, augment)
        ratio, pad, (nh, nw), (top, bottom, left, right) = _geometry((h, w), new_shape, auto, False, scale_up)
        size = (nh + top + bottom, nw + left + right)
        if out_size is None:
            out_size = size
        elif size != out_size:
            raise ValueError("letterbox_batch: image %d ends at %r, the ones before it at %r (rect batches are made per shape)" % (b, size, out_size))
        plan.append(((h0, w0), (h, w), interp1, (nh, nw), top, left, ratio, pad))
        shapes.append(((h0, w0), ((h / h0, w / w0), pad)))
    two_steps = any(p[0] != p[1] and p[1] != p[3] for p in plan)
    if two_steps:
        groups = {}
        for b, p in enumerate(plan):
            groups.setdefault(p[1], []).append(b)
        for (h, w), idx in groups.items():
            iv, il = F.resize_pad_pairs([vs[b] for b in idx], [ls[b] for b in idx], [(h, w, 0, 0, plan[b][2]) for b in idx], (h, w), layout=layout)
            for k, b in enumerate(idx):
                vs[b], ls[b] = iv[k], il[k]
        layout = "chw"
        geom = [(p[3][0], p[3][1], p[4], p[5], LINEAR) for p in plan]
    else:
        geom = [(p[3][0], p[3][1], p[4], p[5], p[2] if p[0] != p[1] else LINEAR) for p in plan]
    ov, ol = F.resize_pad_pairs(vs, ls, geom, out_size, layout=layout, color=color)
    out_labels = None
    if labels is not None:
        if len(labels) != len(plan):
            raise ValueError("letterbox_batch: %d label arrays for %d images" % (len(labels), len(plan)))
        out_labels = [letterbox_labels(x, p[6], p[7], p[1][1], p[1][0]) for x, p in zip(labels, plan)]
    return ov, ol, shapes, out_labels
