"""Seeded cases for the multi-class evaluator (tests/test_map_reference.py on the CPU, tests/test_gpu_evalmap.py on the GPU).

A case is a dict: nc, thresholds, max_num, shapes [(w, h)], labels (per image float32 [k,5]: cls, xc, yc, w, h relative),
dets (per image float32 [n,6] in the ORIGINAL frame: x1, y1, x2, y2, conf, cls, descending conf -- NMS order -- or None).
Detections are jittered copies of ground-truth boxes (now and then with another class) plus clutter; scores are drawn from a
coarse grid so that ties within and across images occur; every coordinate is finite.  Sizes are the smallest at which the
kernel can go wrong: 0 / 1 / 63 / 64 / 65 / 1024 boxes per image (lane stride 64, LDS capacity 1024), max_num 8 and 100, an
image without detections.  The hand-built cases further down each pin one rule of the matching."""
import functools

import numpy as np

IMG1 = (416, 512)                                   # (h, w) of the network input of the letterboxed runs
SHAPES = [(640, 512), (320, 256), (600, 400), (512, 512), (333, 517)]


def thresholds(T):
    return {1: (0.5,), 10: tuple(round(0.5 + 0.05 * i, 2) for i in range(10)),
            16: tuple(round(0.2 + 0.05 * i, 2) for i in range(16))}[T]


MATRIX = {
    # name: (seed, nc, T, max_num, boxes per image, index of the image without detections)
    "nc1_t1_m8": (1, 1, 1, 8, [0, 1, 63, 64, 65], 3),
    "nc3_t10_m100": (2, 3, 10, 100, [65, 64, 63, 1, 0], 4),
    "nc80_t16_m100": (3, 80, 16, 100, [1024, 0, 1, 64, 65], 2),
    "nc1_t10_m100_full": (4, 1, 10, 100, [64, 1024, 65, 63, 1], 4),
    "nc3_t16_m8_full": (5, 3, 16, 8, [1, 65, 1024, 0, 64], 0),
    "nc80_t1_m100": (6, 80, 1, 100, [63, 65, 0, 64, 1], 2),
}


def _image(rng, w, h, k, nc, max_num, empty):
    lab = np.zeros((k, 5), np.float32)
    bw, bh = rng.uniform(6, 60, k), rng.uniform(10, 120, k)
    xc, yc = rng.uniform(bw / 2, w - bw / 2), rng.uniform(bh / 2, h - bh / 2)
    lab[:, 0] = rng.integers(0, nc, k)
    lab[:, 1], lab[:, 2], lab[:, 3], lab[:, 4] = xc / w, yc / h, bw / w, bh / h
    if empty:
        return lab, None
    rows = []
    for j in rng.permutation(k)[:max_num]:
        for _ in range(int(rng.integers(0, 3))):               # 0, 1 or 2 detections on this box
            jit = rng.uniform(-0.15, 0.15, 4) * (bw[j], bh[j], bw[j], bh[j])
            box = np.array([xc[j] - bw[j] / 2, yc[j] - bh[j] / 2, xc[j] + bw[j] / 2, yc[j] + bh[j] / 2]) + jit
            if rng.random() < 0.2:
                box = np.floor(box)                            # integer corners: exact IoU ties
            cls = lab[j, 0] if rng.random() < 0.85 else rng.integers(0, nc)
            rows.append(list(box) + [0.0, cls])
    for _ in range(int(rng.integers(2, 6))):                   # clutter
        x1, y1 = rng.uniform(0, w - 40), rng.uniform(0, h - 40)
        rows.append([x1, y1, x1 + rng.uniform(5, 40), y1 + rng.uniform(5, 40), 0.0, rng.integers(0, nc)])
    d = np.array(rows, np.float32)
    d[:, 0:4:2] = np.clip(d[:, 0:4:2], 0, w)
    d[:, 1:4:2] = np.clip(d[:, 1:4:2], 0, h)
    d[:, 4] = rng.integers(5, 100, d.shape[0]) / np.float32(100)          # a coarse grid: score ties
    d = d[np.argsort(-d[:, 4], kind="stable")][:max_num]
    return lab, d


@functools.lru_cache(maxsize=None)
def case(name):
    seed, nc, T, max_num, boxes, none_at = MATRIX[name]
    rng = np.random.default_rng(seed)
    labels, dets = [], []
    for b, ((w, h), k) in enumerate(zip(SHAPES, boxes)):
        lab, d = _image(rng, w, h, k, nc, max_num, b == none_at)
        labels.append(lab)
        dets.append(d)
    return {"nc": nc, "thresholds": thresholds(T), "max_num": max_num, "shapes": list(SHAPES), "labels": labels, "dets": dets}


def targets_of(labels):
    """the collate contract of the loss: [nt,6] (image in batch, class, xc, yc, w, h), sorted by image"""
    rows = [np.concatenate([np.full((lab.shape[0], 1), b, np.float32), lab], 1) for b, lab in enumerate(labels)]
    return np.concatenate(rows).astype(np.float32).reshape(-1, 6)


def padded_of(dets, max_num, fill=0.0):
    """(out [B, max_num, 6], counts) as dyk_nms leaves them; rows past the count hold `fill`"""
    out = np.full((len(dets), max_num, 6), fill, np.float32)
    counts = [0 if d is None else d.shape[0] for d in dets]
    for b, d in enumerate(dets):
        if d is not None:
            out[b, :counts[b]] = d
    return out, counts


def ratio_pad_of(shape):
    """what the loader records for an image of `shape` (w, h) letterboxed into IMG1"""
    w, h = shape
    gain = min(IMG1[0] / h, IMG1[1] / w)
    return ((gain, gain), ((IMG1[1] - w * gain) / 2, (IMG1[0] - h * gain) / 2))


def letterboxed(c):
    """the case's detections moved onto the network input (fp32), and the per-image ratio_pad that moves them back"""
    rps = [ratio_pad_of(s) for s in c["shapes"]]
    raw = []
    for d, rp in zip(c["dets"], rps):
        if d is None:
            raw.append(None)
            continue
        r = d.copy()
        r[:, 0:4:2] = d[:, 0:4:2] * np.float32(rp[0][0]) + np.float32(rp[1][0])
        r[:, 1:4:2] = d[:, 1:4:2] * np.float32(rp[0][0]) + np.float32(rp[1][1])
        raw.append(r)
    return raw, rps


# ------------------------------------------------------------------------------------------------------------------------
# hand-built cases: one image of 100 x 100 unless stated, boxes given as absolute corners (x1, y1, x2, y2)
def _lab(cls, box, w=100, h=100):
    """a label whose int32 box is exactly floor(box): the corners sit a quarter / a half pixel inside their cell, far from
    any fp32 rounding of the relative form"""
    x1, y1, x2, y2 = box[0] + 0.25, box[1] + 0.25, box[2] + 0.5, box[3] + 0.5
    return [cls, (x1 + x2) / 2 / w, (y1 + y2) / 2 / h, (x2 - x1) / w, (y2 - y1) / h]


def _hand(nc, thr, images):
    """images: list of (labels [(cls, box)], detections [(box, conf, cls)] in NMS order)"""
    labels = [np.array([_lab(c, b) for c, b in labs], np.float32).reshape(-1, 5) for labs, _ in images]
    dets = [np.array([list(b) + [s, c] for b, s, c in ds], np.float32) if ds else None for _, ds in images]
    return {"nc": nc, "thresholds": tuple(thr), "max_num": 8, "shapes": [(100, 100)] * len(images), "labels": labels, "dets": dets}


A, A2, NEAR = (10, 10, 29, 49), (10, 10, 29, 47), (14, 10, 33, 49)
HAND = {
    # AP 5/6 for class 0 (TP, FP, TP over two boxes), AP 0 for class 1 (a box, no detection), nan for class 2: map50 5/12
    "hand_map": _hand(3, (0.5,), [([(0, A), (0, (60, 10, 79, 49)), (1, (40, 60, 59, 89))],
                                  [(A, 0.9, 0), ((0, 60, 9, 69), 0.8, 0), ((60, 10, 79, 49), 0.7, 0)])]),
    # the detection's best box is claimed; its second best (IoU 0.6...) is free: still a false positive
    "second_best": _hand(1, (0.5,), [([(0, A), (0, NEAR)], [(A, 0.9, 0), (A2, 0.8, 0)])]),
    # IoU exactly 0.5: [0,0,9,9] in [0,0,9,19] is 100 / 200 with the pixel-inclusive +1 -- a TP at 0.5; one pixel off is not
    "exact_half": _hand(1, (0.5,), [([(0, (0, 0, 9, 19)), (0, (50, 0, 59, 19))],
                                     [((0, 0, 9, 9), 0.9, 0), ((50, 0, 59, 8), 0.8, 0)])]),
    # a class-1 detection on a class-0 box, and a detection whose class has no box in the image
    "other_class": _hand(3, (0.5,), [([(0, A)], [(A, 0.9, 1), (A, 0.8, 0), (A, 0.7, 2)])]),
    # IoU 0.6 claims the box at 0.5 only; the better detection that follows is a TP at 0.75 and an FP at 0.5
    "per_threshold": _hand(1, (0.5, 0.75), [([(0, A)], [((10, 10, 29, 33), 0.9, 0), (A, 0.8, 0)])]),
    # two identical boxes: the first wins; the next detection has the same argmax (claimed) and does NOT get the second
    "twins": _hand(1, (0.5,), [([(0, A), (0, A)], [(A, 0.9, 0), (A, 0.8, 0)])]),
    # several detections on one box, and a second image whose equal scores must keep image order
    "ties_across_images": _hand(1, (0.5,), [([(0, A)], [(A, 0.9, 0), (A2, 0.5, 0), ((60, 60, 69, 69), 0.5, 0)]),
                                            ([(0, A)], [(A, 0.5, 0), (A2, 0.5, 0)])]),
}
