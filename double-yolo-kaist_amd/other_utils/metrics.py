"""Pedestrian AP@0.5 / log-average miss rate from NMS keep-sets -- same API and results as the reference's
other_utils/metrics.py (voc_ap :7, log_average_miss_rate :31, box_iou :62, compute_ap_lamr :81), so the second half
of the headline metric ("eval AP within +-0.1") can be computed on the GPU box from this framework's detections
without pycocotools.  Host-side numpy by design: the inputs are <= 100 detections per image after NMS.

Differences from the reference, both deliberate:
  * `labels` is not modified (the reference rewrites the caller's arrays in place, so it can be called once only);
  * the per-prediction IoU row and the curve post-processing are vectorised; the greedy matching stays sequential
    because a ground truth claimed by a higher-scoring detection turns later matches into false positives.

`compute_map` (not in the reference, whose multi-class number comes from a pycocotools wrapper) is the host half of the
multi-class evaluator dyk.evalmap.DetectionEvaluator: per-class AP / LAMR at several IoU thresholds and their means from the
per-detection match records dyk_eval_match writes on the device, through the same `voc_ap` / `log_average_miss_rate`.

`coco_accumulate` is the host half of dyk.evalmap.CocoEvaluator: the accumulation and the twelve summary numbers of the COCO
bbox protocol (what the reference's training harness reads from pycocotools) from the records dyk_eval_match_coco writes.
"""
import math

import numpy as np

IOU_THRESHOLD = 0.5


def voc_ap(recall, precision):
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([0.0], precision, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]             # precision envelope
    step = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return np.sum((mrec[step] - mrec[step - 1]) * mpre[step])


def log_average_miss_rate(recall, fp_cumsum, num_imgs):
    fppi = fp_cumsum / float(num_imgs)
    mr = 1 - recall
    x = np.concatenate(([-1.0], fppi))
    y = np.concatenate(([1.0], mr))
    # fppi is non-decreasing: the last index with x <= ref is a right-sided binary search
    pos = np.searchsorted(x, np.logspace(-2.0, 0.0, num=9), side="right") - 1
    lamr = math.exp(np.mean(np.log(np.maximum(1e-10, y[pos]))))
    return lamr, fppi, mr


def box_iou(box1, box2):
    """box1 [1,4] (or [m,4]) xyxy, box2 [n,4] xyxy -> [m,n]; extents are pixel-inclusive (+1)."""
    area1 = (box1[:, 2] - box1[:, 0] + 1) * (box1[:, 3] - box1[:, 1] + 1)
    area2 = (box2[:, 2] - box2[:, 0] + 1) * (box2[:, 3] - box2[:, 1] + 1)
    wh = np.minimum(box1[:, None, 2:], box2[:, 2:]) - np.maximum(box1[:, None, :2], box2[:, :2]) + 1
    inter = np.prod(np.clip(wh, 0, 1e5), axis=2)
    return inter / (area1[:, None] + area2 - inter)


def _absolute_xyxy(labels, shapes):
    assert len(labels) == len(shapes), "label's len != shape's len"
    out = []
    for lab, (w, h) in zip(labels, shapes):
        lab = np.array(lab, dtype=np.float32, copy=True)
        lab[:, [1, 3]] *= w
        lab[:, [2, 4]] *= h
        lab[:, 1] -= lab[:, 3] / 2
        lab[:, 2] -= lab[:, 4] / 2
        lab[:, 3] += lab[:, 1]
        lab[:, 4] += lab[:, 2]
        out.append(lab)
    return out


def compute_ap_lamr(preds, labels, shapes):
    """preds: list of dicts {img_id, conf, bbox (float32 xyxy)} sorted by descending confidence;
    labels: per image [k,5] (class/flag, xc, yc, w, h) relative; shapes: per image (w, h).
    Returns {'recall','precision','fppi','mr','ap','lamr'}."""
    gts = [lab[:, 1:].astype(np.int32) for lab in _absolute_xyxy(labels, shapes)]
    claimed = [np.zeros(g.shape[0], dtype=bool) for g in gts]
    nt = sum(g.shape[0] for g in gts)
    tp = np.zeros(len(preds), dtype=np.int32)
    for n, pr in enumerate(preds):
        i = pr["img_id"]
        iou = box_iou(pr["bbox"].reshape(-1, 4), gts[i])[0]
        k = int(np.argmax(iou))
        if iou[k] >= IOU_THRESHOLD and not claimed[i][k]:
            claimed[i][k] = True
            tp[n] = 1
    tp_cum = np.cumsum(tp)
    fp_cum = np.cumsum(1 - tp)
    recall = tp_cum / nt
    precision = tp_cum / (tp_cum + fp_cum)
    ap = voc_ap(recall, precision)
    lamr, fppi, mr = log_average_miss_rate(recall, fp_cum, len(labels))
    return {"recall": recall, "precision": precision, "fppi": fppi, "mr": mr, "ap": ap, "lamr": lamr}


def compute_map(conf, cls, tp_mask, n_gt_per_class, num_imgs, iou_thresholds=(0.5,), names=None):
    """Per-class AP / LAMR at one or several IoU thresholds, and their means, from per-detection match records.

    conf [n] scores, cls [n] class indices, tp_mask [n] uint32 with bit t set when the detection is a true positive at
    iou_thresholds[t] -- the records of dyk.evalmap.DetectionEvaluator (dyk_eval_match), in append order: image, then
    rank within the image.  n_gt_per_class [nc] ground-truth boxes per class, num_imgs the images evaluated.

    The records are sorted stably by descending conf (what Python's stable sort(reverse=True) gives evaluate.py:114:
    equal scores keep append order); per class and threshold the cumulative TP / FP, recall and precision go through
    `voc_ap` and `log_average_miss_rate` above.  Returns a dict:
      ap, lamr [nc, T]     nan for a class without ground truth, AP 0 / LAMR 1 for one with ground truth and no detection
      map                  mean of ap over the thresholds and the classes that have ground truth (nan when none has)
      map50                the same at the threshold 0.5 (key present only when 0.5 is among iou_thresholds)
      recall, precision    [nc][T] lists of the per-detection curves
      summary              the table as text, rows labelled by `names`

    This is the VOC / KAIST rule of compute_ap_lamr applied per class: a detection is matched to the box of its class
    with the largest IoU (np.argmax) and is a false positive when that box is already claimed -- not COCO's
    best-unclaimed rule; AP is the continuous `voc_ap` integral, not COCO's 101-point interpolation; there are no crowd
    regions and no area ranges.  The numbers are therefore not comparable with published COCO figures.  For the COCO
    protocol itself use dyk.evalmap.CocoEvaluator (`coco_accumulate` below)."""
    conf, cls, tp_mask = np.asarray(conf), np.asarray(cls).astype(np.int64), np.asarray(tp_mask).astype(np.uint32)
    n_gt = np.asarray(n_gt_per_class, dtype=np.int64)
    nc, T = n_gt.shape[0], len(iou_thresholds)
    order = np.argsort(-conf.astype(np.float64), kind="stable")
    cls, tp_mask = cls[order], tp_mask[order]
    ap, lamr = np.full((nc, T), np.nan), np.full((nc, T), np.nan)
    recall = [[None] * T for _ in range(nc)]
    precision = [[None] * T for _ in range(nc)]
    for c in np.nonzero(n_gt > 0)[0]:
        bits = tp_mask[cls == c]
        for t in range(T):
            tp = ((bits >> np.uint32(t)) & np.uint32(1)).astype(np.int32)
            tp_cum, fp_cum = np.cumsum(tp), np.cumsum(1 - tp)
            rec = tp_cum / n_gt[c]
            prec = tp_cum / (tp_cum + fp_cum)
            recall[c][t], precision[c][t] = rec, prec
            ap[c, t] = voc_ap(rec, prec)
            lamr[c, t] = log_average_miss_rate(rec, fp_cum, num_imgs)[0]
    has = n_gt > 0
    res = {"ap": ap, "lamr": lamr, "recall": recall, "precision": precision,
           "map": float(ap[has].mean()) if has.any() else float("nan")}
    at50 = [t for t, v in enumerate(iou_thresholds) if float(v) == 0.5]
    if at50:
        res["map50"] = float(ap[has, at50[0]].mean()) if has.any() else float("nan")
    label = (lambda c: str(names[c])) if names is not None else (lambda c: "class %d" % c)
    rows = ["%-20s %8s %8s %8s" % ("class", "boxes", "AP@%.2f" % float(iou_thresholds[0]), "AP mean")]
    rows += ["%-20s %8d %8.4f %8.4f" % (label(c), n_gt[c], ap[c, 0], ap[c].mean()) for c in range(nc)]
    rows.append("%-20s %8d %8s %8.4f" % ("all (VOC-style mAP)", n_gt.sum(), "", res["map"]))
    res["summary"] = "\n".join(rows)
    return res


# ------------------------------------------------------------------------------------------------------------------------
# COCO protocol: the host half of dyk.evalmap.CocoEvaluator (the device half is dyk_eval_match_coco; the protocol is stated
# in include/dyk_hip.h).  Written from the published algorithm; no COCO tool is installed where this project runs, so
# agreement with pycocotools is derived (tests/coco_ref.py and its hand-worked cases), not measured.
COCO_IOU_THRESHOLDS = tuple(float(v) for v in np.linspace(0.5, 0.95, 10))
COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
COCO_RECALL_GRID = np.linspace(0.0, 1.0, 101)


def _coco_mean(cells):
    cells = cells[cells > -1]
    return float(cells.mean()) if cells.size else -1.0


def coco_accumulate(conf, cls, img, rank, dtm, dtig, n_gt_ka, iou_thresholds, area_ranges, max_dets, names=None):
    """The accumulation and the summary of the COCO bbox protocol from per-detection match records.

    conf, cls, img, rank [n]: score, class, image (in update order) and rank within image and class of every detection;
    dtm, dtig [n, A] uint32: bit t set when the detection is matched / ignored at (area range a, iou_thresholds[t]) -- the
    records of dyk.evalmap.CocoEvaluator (dyk_eval_match_coco); n_gt_ka [K, A]: the non-ignored ground-truth boxes.

    Per class k, area range a and M in max_dets: the detections of the class with rank < M, by image, then rank, stably
    sorted by descending score; tp = cumsum(matched & ~ignored), fp = cumsum(~matched & ~ignored); recall tp / npig,
    precision tp / (fp + tp + spacing(1)) made non-increasing from the right and read at the first index whose recall
    reaches each of the 101 grid points (0 past the end).  A cell without non-ignored ground truth stays -1 and is left
    out of every mean.  Returns a dict:
      precision [T, 101, K, A, M], recall [T, K, A, M]
      stats         the twelve numbers of the protocol's summary, in its order: AP, AP@.5, AP@.75, AP small / medium /
                    large, AR at max_dets[0] / [1] / [2], AR small / medium / large.  Area ranges 1..3 are small / medium /
                    large; AP and the area lines use the last max_dets; the .5 / .75 lines use those thresholds when they
                    are among iou_thresholds; whatever does not exist is -1
      ap_per_class  [K] AP over all thresholds, area range 0, the last max_dets (-1 without ground truth)
      summary       the twelve lines as text (and one line per class when `names` is given)"""
    conf, cls = np.asarray(conf, dtype=np.float64), np.asarray(cls).astype(np.int64)
    img, rank = np.asarray(img).astype(np.int64), np.asarray(rank).astype(np.int64)
    n_gt = np.asarray(n_gt_ka, dtype=np.int64)
    K, A = n_gt.shape
    T, M = len(iou_thresholds), len(max_dets)
    dtm, dtig = np.asarray(dtm).astype(np.uint32).reshape(-1, A), np.asarray(dtig).astype(np.uint32).reshape(-1, A)
    order = np.lexsort((rank, img, -conf))                   # stable: score descending, then image, then rank
    cls, rank, dtm, dtig = cls[order], rank[order], dtm[order], dtig[order]
    by_class = np.argsort(cls, kind="stable")
    bounds = np.searchsorted(cls[by_class], np.arange(K + 1))
    bit = np.arange(T, dtype=np.uint32)[:, None]
    precision, recall = -np.ones((T, 101, K, A, M)), -np.ones((T, K, A, M))
    for k in np.nonzero(n_gt.any(axis=1))[0]:
        mine = by_class[bounds[k]:bounds[k + 1]]
        for mi, mx in enumerate(max_dets):
            sel = mine[rank[mine] < mx]
            nd = sel.shape[0]
            for a in np.nonzero(n_gt[k])[0]:
                if nd == 0:
                    precision[:, :, k, a, mi], recall[:, k, a, mi] = 0.0, 0.0
                    continue
                matched = ((dtm[sel, a][None, :] >> bit) & 1).astype(bool)           # [T, nd]
                ignored = ((dtig[sel, a][None, :] >> bit) & 1).astype(bool)
                tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                rc = tp / n_gt[k, a]
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                recall[:, k, a, mi] = rc[:, -1]
                for t in range(T):
                    at = np.searchsorted(rc[t], COCO_RECALL_GRID, side="left")
                    inside = at < nd
                    q = np.zeros(101)
                    q[inside] = pr[t, at[inside]]
                    precision[t, :, k, a, mi] = q

    def t_of(v):
        hits = [t for t, x in enumerate(iou_thresholds) if float(x) == v]
        return hits[0] if hits else None

    def ap(t=slice(None), a=0):
        return -1.0 if t is None or a >= A else _coco_mean(precision[t, :, :, a, M - 1])

    def ar(a=0, m=M - 1):
        return -1.0 if a >= A or m >= M else _coco_mean(recall[:, :, a, m])

    stats = [ap(), ap(t_of(0.5)), ap(t_of(0.75)), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3)]
    ap_per_class = np.array([_coco_mean(precision[:, :, k, 0, M - 1]) for k in range(K)])
    span = "%.2f:%.2f" % (float(iou_thresholds[0]), float(iou_thresholds[-1]))
    dets = lambda m: int(max_dets[m]) if m < M else -1
    label = ("all", "small", "medium", "large")
    lines = [("Average Precision", "(AP)", span, 0, M - 1), ("Average Precision", "(AP)", "0.50", 0, M - 1),
             ("Average Precision", "(AP)", "0.75", 0, M - 1)]
    lines += [("Average Precision", "(AP)", span, a, M - 1) for a in (1, 2, 3)]
    lines += [("Average Recall", "(AR)", span, 0, m) for m in (0, 1, 2)] + [("Average Recall", "(AR)", span, a, M - 1) for a in (1, 2, 3)]
    rows = [" %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f" % (what, tag, iou, label[a], dets(m), v)
            for (what, tag, iou, a, m), v in zip(lines, stats)]
    if names is not None:
        rows += [" %-20s %8d boxes  AP = %0.3f" % (str(names[k]), n_gt[k, 0], ap_per_class[k]) for k in range(K)]
    return {"precision": precision, "recall": recall, "stats": stats, "ap_per_class": ap_per_class, "summary": "\n".join(rows)}
