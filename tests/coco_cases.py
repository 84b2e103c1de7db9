"""Seeded cases for the COCO-protocol evaluator (tests/test_coco_reference.py on the CPU, tests/test_gpu_evalmap_coco.py on the
GPU), in the form of tests/map_cases.py: a case is a dict with nc, max_num, shapes [(w, h)], labels (per image float32 [k,5]:
cls, xc, yc, w, h relative) and dets (per image float32 [n,6] in the ORIGINAL frame, descending score, or None), plus the
protocol's parameters when they are not the defaults (thresholds, areas, max_dets).

Box sides are log-uniform in [8, 220] px with aspect exp(U(-0.5, 0.5)), so every area range holds boxes; the rest is as
map_cases._image.  Sizes are the smallest at which the kernel can go wrong: 0 / 1 / 63 / 64 / 65 / 1024 boxes per image (lane
stride 64, LDS capacity 1024), max_num 8 / 100 / 160 (above max_det = 100), an image without detections.

The hand cases further down pin one rule each and carry their answer, worked out by hand, in `check_hand`: 128 x 128 images,
coordinates on the 1/128 grid, so every fp32 step of the protocol is exact."""
import functools

import numpy as np

from map_cases import SHAPES

MATRIX = {
    # name: (seed, nc, max_num, boxes per image, index of the image without detections)
    "nc1_m8": (1, 1, 8, [0, 1, 63, 64, 65], 3),
    "nc3_m100": (2, 3, 100, [65, 64, 63, 1, 0], 4),
    "nc80_m100": (3, 80, 100, [1024, 0, 1, 64, 65], 2),
    "nc1_m160": (4, 1, 160, [64, 1024, 65, 63, 1], 4),
    "nc3_m8": (5, 3, 8, [1, 65, 1024, 0, 64], 0),
}


def _image(rng, w, h, k, nc, max_num, empty):
    lab = np.zeros((k, 5), np.float32)
    side, asp = np.exp(rng.uniform(np.log(8), np.log(220), k)), np.exp(rng.uniform(-0.5, 0.5, k))
    bw, bh = np.minimum(side * asp, w), np.minimum(side / asp, h)
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
            cls = lab[j, 0] if rng.random() < 0.85 else rng.integers(0, nc)
            rows.append(list(box) + [0.0, cls])
    for _ in range(int(rng.integers(2, 6))):                   # clutter
        s = np.exp(rng.uniform(np.log(8), np.log(220)))
        x1, y1 = rng.uniform(0, w - 8), rng.uniform(0, h - 8)
        rows.append([x1, y1, x1 + s, y1 + s * np.exp(rng.uniform(-0.5, 0.5)), 0.0, rng.integers(0, nc)])
    d = np.array(rows, np.float32)
    d[:, 0:4:2] = np.clip(d[:, 0:4:2], 0, w)
    d[:, 1:4:2] = np.clip(d[:, 1:4:2], 0, h)
    d[:, 4] = rng.integers(5, 100, d.shape[0]) / np.float32(100)          # a coarse grid: score ties
    d = d[np.argsort(-d[:, 4], kind="stable")][:max_num]
    return lab, d


@functools.lru_cache(maxsize=None)
def case(name):
    seed, nc, max_num, boxes, none_at = MATRIX[name]
    rng = np.random.default_rng(seed)
    labels, dets = [], []
    for b, ((w, h), k) in enumerate(zip(SHAPES, boxes)):
        lab, d = _image(rng, w, h, k, nc, max_num, b == none_at)
        labels.append(lab)
        dets.append(d)
    return {"nc": nc, "max_num": max_num, "shapes": list(SHAPES), "labels": labels, "dets": dets}


def custom(name, thresholds, areas):
    """a matrix case under other protocol parameters"""
    c = dict(case(name))
    c["thresholds"], c["areas"] = tuple(thresholds), tuple(areas)
    return c


# ------------------------------------------------------------------------------------------------------------------------
# hand cases: 128 x 128 images; ground truth as (class, (x, y, w, h)) in pixels, detections as ((x1, y1, x2, y2), score, class)
def _hand(nc, images, **params):
    labels, dets = [], []
    for labs, ds in images:
        labels.append(np.array([[c, (x + w / 2) / 128, (y + h / 2) / 128, w / 128, h / 128] for c, (x, y, w, h) in labs],
                               np.float32).reshape(-1, 5))
        dets.append(np.array([list(b) + [s, c] for b, s, c in ds], np.float32) if ds else None)
    c = {"nc": nc, "max_num": max([8] + [d.shape[0] for d in dets if d is not None]), "shapes": [(128, 128)] * len(images),
         "labels": labels, "dets": dets}
    c.update(params)
    return c


def _xyxy(x, y, w, h):
    return (x, y, x + w, y + h)


G = (10, 10, 20, 40)                                             # 800 px: "all" and "small"
FAR = [((100 + (i % 4) * 6, 2 + (i // 4) * 5, 104 + (i % 4) * 6, 5 + (i // 4) * 5), 0.99 - 0.004 * i, 0) for i in range(100)]
GRID = [(0, (4 + (i % 4) * 30, 4 + (i // 4) * 30, 8, 8)) for i in range(12)]
HAND = {
    "twins": _hand(1, [([(0, G), (0, G)], [(_xyxy(*G), 0.9, 0), (_xyxy(*G), 0.8, 0)])]),
    # IoU with row 0: 1 and 0.95; with row 1 (4 px to the right): 2/3 and 608/952 = 0.6387
    "second_best": _hand(1, [([(0, G), (0, (14, 10, 20, 40))], [(_xyxy(*G), 0.9, 0), ((10, 10, 30, 48), 0.8, 0)])]),
    "exact_half": _hand(1, [([(0, (10, 10, 10, 20)), (0, (50, 10, 10, 20))],
                             [((10, 10, 20, 20), 0.9, 0), ((50, 10, 60, 19), 0.8, 0)])]),
    "thr_one": _hand(1, [([(0, G)], [(_xyxy(*G), 0.9, 0)])], thresholds=(0.5, 1.0)),
    "area_edges": _hand(1, [([(0, (0, 0, 32, 32)), (0, (32, 32, 96, 96))],
                             [((0, 0, 32, 32), 0.9, 0), ((32, 32, 128, 128), 0.8, 0)])]),
    # a 40 x 40 box (medium) under the best-scored detection, a 16 x 16 one (small) under the other
    "ignored_match": _hand(1, [([(0, (10, 10, 40, 40)), (0, (80, 80, 16, 16))],
                                [((10, 10, 50, 50), 0.9, 0), ((80, 80, 96, 96), 0.8, 0)])]),
    # a 32 x 32 detection: IoU 1024/1120 = 0.914 with row 0 (1120 px, not small), 640/1024 = 0.625 with row 1 (640 px)
    "prefer_kept": _hand(1, [([(0, (10, 10, 32, 35)), (0, (10, 10, 32, 20))], [((10, 10, 42, 42), 0.9, 0)])]),
    "unmatched_area": _hand(1, [([(0, (100, 100, 20, 20))], [((10, 10, 20, 20), 0.9, 0), ((30, 30, 80, 80), 0.8, 0)])]),
    # a hundred far-away detections in front of the one that sits on the box
    "rank_cut": _hand(1, [([(0, G)], FAR + [(_xyxy(*G), 0.5, 0)])]),
    "max_dets": _hand(1, [(GRID, [(_xyxy(*g), 0.9 - 0.01 * i, 0) for i, (_, g) in enumerate(GRID)])]),
    # all scores equal: image 0 (FP, then TP), then image 1 (TP): precision 0, 1/2, 2/3
    "ties_across_images": _hand(1, [([(0, G)], [((60, 60, 80, 80), 0.5, 0), (_xyxy(*G), 0.5, 0)]),
                                    ([(0, G)], [(_xyxy(*G), 0.5, 0)])]),
    "no_gt_class": _hand(3, [([(0, G), (1, (60, 60, 20, 40))], [(_xyxy(*G), 0.9, 0), ((60, 10, 80, 50), 0.8, 2)])]),
    "half_even": _hand(1, [([(0, (10, 20, 32, 32))], [((10.5, 20.5, 41.5, 51.5), 0.9, 0)])]),
    "hand_ap": _hand(1, [([(0, G), (0, (60, 60, 20, 40))],
                          [(_xyxy(*G), 0.9, 0), ((60, 10, 80, 50), 0.8, 0), ((60, 60, 80, 100), 0.7, 0)])]),
}
ALL = 0x3ff                                                      # the ten default thresholds


def check_hand(name, rec, stats, npig, round_boxes=True):
    """the written answers.  rec: the record fields (match: rows of the image's own labels), stats: the twelve numbers"""
    dtm, dtig, match = rec["dtm"], rec["dtig"], rec["match"]
    near = lambda v, want: abs(v - want) < 1e-12                 # np.spacing(1) in the precision's denominator
    if name == "twins":                  # the first detection takes the LATER of two equal boxes, the second the other: both TP
        assert match[:, 0, :].tolist() == [[1] * 10, [0] * 10] and dtm[:, 0].tolist() == [ALL, ALL] and near(stats[0], 1.0)
    elif name == "second_best":          # row 0 is claimed; row 1 (IoU 0.6387) is free at 0.5, 0.55 and 0.6
        assert match[0, 0].tolist() == [0] * 10 and match[1, 0].tolist() == [1, 1, 1] + [-1] * 7 and dtm[1, 0] == 7
    elif name == "exact_half":           # 100 / 200 matches at 0.5 and nowhere else; 90 / 200 nowhere
        assert dtm[:, 0].tolist() == [1, 0]
    elif name == "thr_one":              # IoU 1.0 against min(1.0, 1 - 1e-10)
        assert dtm[0, 0] == 3 and match[0, 0].tolist() == [0, 0]
    elif name == "area_edges":           # 1024 px is small AND medium, 9216 px is medium AND large
        assert npig.tolist() == [[2, 1, 2, 1]]
        assert dtm.tolist() == [[ALL] * 4] * 2 and dtig.tolist() == [[0, 0, 0, ALL], [0, ALL, 0, 0]]
    elif name == "ignored_match":        # in "small" the best-scored detection sits on an ignored box: not an FP, AP small stays 1
        assert dtm[0].tolist() == [ALL] * 4 and dtig[0].tolist() == [0, ALL, 0, ALL] and near(stats[3], 1.0) and near(stats[0], 1.0)
    elif name == "prefer_kept":          # "all": the better row 0.  "small": the kept row 1 while 0.625 suffices, then the ignored row 0
        assert match[0, 0].tolist() == [0] * 9 + [-1] and match[0, 1].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, -1]
        assert dtm[0, :2].tolist() == [0x1ff, 0x1ff] and dtig[0, :2].tolist() == [0, 0x1f8]
    elif name == "unmatched_area":       # 100 px is small, 2500 px is medium: ignored outside, a false positive inside
        assert (dtm == 0).all() and dtig.tolist() == [[0, 0, ALL, ALL], [0, ALL, 0, ALL]]
    elif name == "rank_cut":             # rank 100 takes no part
        assert rec["rank"][100] == 100 and (dtm == 0).all() and (dtig[100] == 0).all() and (match == -1).all() and stats[8] == 0.0
    elif name == "max_dets":
        assert near(stats[6], 1 / 12) and near(stats[7], 10 / 12) and stats[8] == 1.0 and near(stats[0], 1.0)
    elif name == "ties_across_images":
        assert rec["img"].tolist() == [0, 0, 1] and dtm[:, 0].tolist() == [0, ALL, ALL] and near(stats[0], 2 / 3)
    elif name == "no_gt_class":          # class 0: 1, class 1: 0, class 2 (no ground truth) left out
        assert npig[:, 0].tolist() == [1, 1, 0] and near(stats[0], 0.5) and stats[8] == 0.5
    elif name == "half_even":
        assert rec["box"][0].tolist() == ([10.0, 20.0, 42.0, 52.0] if round_boxes else [10.5, 20.5, 41.5, 51.5])
        assert rec["darea"][0] == (1024.0 if round_boxes else 961.0) and dtm[0, 0] == (ALL if round_boxes else 0x1ff)
    elif name == "hand_ap":              # TP, FP, TP over two boxes: precision 1 up to recall 0.5 (51 points), then 2/3 (50 points)
        assert dtm[:, 0].tolist() == [ALL, 0, ALL]
        assert near(stats[0], (51 + 50 * (2 / 3)) / 101) and near(stats[1], (51 + 50 * (2 / 3)) / 101) and stats[8] == 1.0
    else:
        raise KeyError(name)
