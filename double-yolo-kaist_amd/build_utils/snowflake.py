"""The reference's "snowflake" input transform (reference build_utils/snowflake.py:7-93) under its names and signatures, with
the image work on the MI355X: CLAHE of every channel of the visible and the LWIR image (dyk_clahe, OpenCV's 8-bit rule,
include/dyk_hip.h) and `n_snow` square cut-outs zeroed in both (dyk_cutout_rects); labels that the cut-outs cover too much
are dropped.

Images are uint8 device tensors in the loader's planar layout, [3,H,W] or [B,3,H,W]; labels stay on the host, where the
loader holds them.  `random_cut_box` and `cover_iou` are host numpy and draw / compute exactly what the reference does, so
seeding `np.random` reproduces its boxes.  Nothing here synchronises the device: the rectangles go up in one small copy.
Importing this module needs no cv2.

Three things the reference does are kept on purpose, because a model trained with it saw them:
  * snowflake_cutout draws the boxes with w = rows and h = cols (snowflake.py:73-75) and scales the labels alike (:79-80), so on
    a non-square image the x range of the boxes is the image height;
  * the boxes are applied as slices [ymin:ymax, xmin:xmax]: the upper ends are exclusive and numpy clips them (:88-91);
  * cover_iou clips each side of an intersection to [0, M], M the number of boxes (:41-42).
"""
import numpy as np
import torch

from build_utils.utils import xywh2xyxy


def random_cut_box(w: int, h: int, n: int = 10, step: int = 32):
    """n boxes (xmin, ymin, xmax, ymax) of side `step`, float64 [n,4], from ONE np.random.rand(n, 2) call: the corner uniform
    in [0, w-1] x [0, h-1], the far corner clipped to w-1 / h-1, everything floored (snowflake.py:18-25)"""
    lo = np.random.rand(n, 2) * np.array([w - 1, h - 1], dtype=np.float64)
    hi = np.stack((np.clip(lo[:, 0] + step - 1, 0, w - 1), np.clip(lo[:, 1] + step - 1, 0, h - 1)), 1)
    return np.floor(np.concatenate((lo, hi), 1))


def cover_iou(box1: np.ndarray, box2: np.ndarray):
    """[N,M]: the part of label box1[i] (xyxy) that cut box2[j] covers, over the label's area (floored at 1).  Each side of
    the intersection is clipped to [0, M] with M = len(box2) -- the reference's clip bound is the number of boxes, not a
    length (snowflake.py:41-42); kept."""
    m = np.shape(box2)[0]
    area = np.maximum((box1[:, 2] - box1[:, 0]) * (box1[:, 3] - box1[:, 1]), np.ones(np.shape(box1)[0]))
    sides = np.minimum(box1[:, None, 2:], box2[:, 2:]) - np.maximum(box1[:, None, :2], box2[:, :2])
    return np.prod(np.clip(sides, 0, m), axis=2) / area[:, None]


def clahe_image(v_img, l_img, clip_limit=1.0, tile_grid_size=(4, 4)):
    """CLAHE of every channel of both images: device uint8 [3,H,W] or [B,3,H,W] -> two new tensors"""
    from dyk.functional import clahe
    return clahe(v_img, clip_limit, tile_grid_size), clahe(l_img, clip_limit, tile_grid_size)


def _host_labels(labels):
    return labels.numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)


def _draw(labels, rows, cols, xywh, label_thr, step, n_snow):
    """the host half of one image (snowflake.py:73-86): -> (boxes float64 [n_snow,4], keep mask over the labels [n,5])"""
    w, h = rows, cols                                            # the reference's naming: np.shape(img)[:2] of an HWC image
    boxes = random_cut_box(w, h, n_snow, step)
    lab = _host_labels(labels)
    if xywh:
        xyxy = xywh2xyxy(lab[:, 1:])
        xyxy[:, [0, 2]] *= w
        xyxy[:, [1, 3]] *= h
    else:
        xyxy = lab[:, 1:]
    return boxes, np.sum(cover_iou(xyxy, boxes), axis=1) < label_thr


def snowflake_cutout(v_img, l_img, labels, xywh: bool = True, clahe: bool = True, label_thr: float = 0.35, n_thr: int = 6,
                     step: int = 16, n_snow: int = 25, clip_limit=1.0, grid_size=(4, 4)):
    """One pair: device uint8 [3,H,W] images, host labels [n,5] (class, then xywh normalised or xyxy in pixels; numpy or CPU
    tensor) -> (v, l, labels).  With clahe the images are new tensors, otherwise the cut-outs go into the ones given, as in
    the reference.  More than n_thr labels: no cut-outs, every label kept."""
    from dyk.functional import cutout
    if v_img.dim() != 3 or v_img.shape != l_img.shape:
        raise ValueError("snowflake_cutout: two [3,H,W] images of one shape, got %s and %s" % (tuple(v_img.shape), tuple(l_img.shape)))
    if clahe:
        v_img, l_img = clahe_image(v_img, l_img, clip_limit, grid_size)
    if labels.shape[0] <= n_thr:
        boxes, keep = _draw(labels, int(v_img.shape[1]), int(v_img.shape[2]), xywh, label_thr, step, n_snow)
        labels = labels[torch.from_numpy(keep)] if isinstance(labels, torch.Tensor) else labels[keep]
        rects = torch.from_numpy(boxes.astype(np.int32)).to(v_img.device, non_blocking=True)
        cutout(v_img, rects)
        cutout(l_img, rects)
    return v_img, l_img, labels


def snowflake_batch(v_imgs, l_imgs, targets, xywh: bool = True, clahe: bool = True, label_thr: float = 0.35, n_thr: int = 6,
                    step: int = 16, n_snow: int = 25, clip_limit=1.0, grid_size=(4, 4)):
    """snowflake_cutout of a whole batch after `.to(device)`: device uint8 [B,3,H,W] batches and the collate function's host
    targets [nt,6] (image, class, then xywh normalised or xyxy in pixels) -> (v, l, targets), the targets filtered, rows in
    their order.  One dyk_clahe launch pair and one dyk_cutout_rects launch per stream for the whole batch.  The images are
    taken in order 0..B-1 and each one with at most n_thr labels draws its boxes with one np.random.rand call, as B calls
    of snowflake_cutout would; an image with more labels gets empty rectangles and keeps its labels."""
    from dyk.functional import cutout
    if v_imgs.dim() != 4 or v_imgs.shape != l_imgs.shape:
        raise ValueError("snowflake_batch: two [B,3,H,W] batches of one shape, got %s and %s" % (tuple(v_imgs.shape), tuple(l_imgs.shape)))
    if clahe:
        v_imgs, l_imgs = clahe_image(v_imgs, l_imgs, clip_limit, grid_size)
    B, rows, cols = int(v_imgs.shape[0]), int(v_imgs.shape[2]), int(v_imgs.shape[3])
    t = _host_labels(targets)
    keep = np.ones(t.shape[0], dtype=bool)
    rects = np.zeros((B, n_snow, 4), dtype=np.int32)             # all zero: an empty rectangle, nothing is cut
    for b in range(B):
        mine = np.nonzero(t[:, 0] == b)[0]
        if mine.shape[0] <= n_thr:
            boxes, keep[mine] = _draw(t[mine, 1:], rows, cols, xywh, label_thr, step, n_snow)
            rects[b] = boxes.astype(np.int32)
    rects = torch.from_numpy(rects).to(v_imgs.device, non_blocking=True)
    cutout(v_imgs, rects)
    cutout(l_imgs, rects)
    return v_imgs, l_imgs, (targets[torch.from_numpy(keep)] if isinstance(targets, torch.Tensor) else targets[keep])
