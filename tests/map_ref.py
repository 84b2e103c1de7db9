"""The yardstick of the multi-class evaluator (dyk_eval_match + other_utils.metrics.compute_map): a deliberately plain numpy
restatement.  For each class and each IoU threshold it runs the sequential loop of other_utils.metrics.compute_ap_lamr over
that class's detections and that class's labels -- the same `box_iou`, the same `_absolute_xyxy` and int32 truncation, the
same argmax-then-claimed rule -- with one addition: a detection in an image that holds no box of its class is a false
positive (compute_ap_lamr would take np.argmax of an empty row there).

It shares no code with compute_map beyond `voc_ap` and `log_average_miss_rate`.

Inputs: dets   per image a float32 [n,6] array (x1, y1, x2, y2 in the original frame, conf, cls) in NMS order, or None
        labels per image a float32 [k,5] array (cls, xc, yc, w, h; relative)
        shapes per image (width, height)
"""
import numpy as np

from other_utils.metrics import _absolute_xyxy, box_iou, log_average_miss_rate, voc_ap


def evaluate(dets, labels, shapes, nc, thresholds):
    B = len(labels)
    assert len(dets) == B == len(shapes)
    first = np.concatenate(([0], np.cumsum([0 if d is None else d.shape[0] for d in dets]))).astype(np.int64)
    row0 = np.concatenate(([0], np.cumsum([lab.shape[0] for lab in labels]))).astype(np.int64)
    n, T = int(first[-1]), len(thresholds)
    rec = {"conf": np.zeros(n, np.float32), "cls": np.zeros(n, np.int32), "tp_mask": np.zeros(n, np.uint32),
           "match": np.full(n, -1, np.int32), "iou": np.zeros(n, np.float64), "box": np.zeros((n, 4), np.float32)}
    for b, d in enumerate(dets):
        if d is not None:
            s = slice(first[b], first[b + 1])
            rec["conf"][s], rec["cls"][s], rec["box"][s] = d[:, 4], d[:, 5].astype(np.int32), d[:, :4]
    res = {"records": rec, "ap": np.full((nc, T), np.nan), "lamr": np.full((nc, T), np.nan), "curves": {}}
    for c in range(nc):
        # this class's labels per image (and the row each one has in the batch's targets), this class's detections
        rows = [np.nonzero(lab[:, 0].astype(np.int32) == c)[0] for lab in labels]
        labs = [lab[r] for lab, r in zip(labels, rows)]
        gts = [lab[:, 1:].astype(np.int32) for lab in _absolute_xyxy(labs, shapes)]
        nt = sum(g.shape[0] for g in gts)
        preds = []
        for b, d in enumerate(dets):
            if d is None:
                continue
            for i in range(d.shape[0]):
                if int(d[i, 5]) == c:
                    preds.append({"img_id": b, "conf": float(d[i, 4]), "bbox": d[i, :4], "rec": int(first[b]) + i})
        preds.sort(key=lambda q: q["conf"], reverse=True)
        for t, thr in enumerate(thresholds):
            claimed = [np.zeros(g.shape[0], dtype=bool) for g in gts]
            tp = np.zeros(len(preds), dtype=np.int32)
            for j, pr in enumerate(preds):
                i = pr["img_id"]
                if gts[i].shape[0] == 0:
                    continue                                   # the one addition: nothing of this class here
                iou = box_iou(pr["bbox"].reshape(-1, 4), gts[i])[0]
                k = int(np.argmax(iou))
                if t == 0:
                    rec["match"][pr["rec"]] = row0[i] + rows[i][k]
                    rec["iou"][pr["rec"]] = iou[k]
                if iou[k] >= thr and not claimed[i][k]:
                    claimed[i][k] = True
                    tp[j] = 1
                    rec["tp_mask"][pr["rec"]] |= np.uint32(1 << t)
            if nt == 0:
                continue                                       # no ground truth of this class anywhere: AP undefined (nan)
            tp_cum = np.cumsum(tp)
            fp_cum = np.cumsum(1 - tp)
            recall = tp_cum / nt
            precision = tp_cum / (tp_cum + fp_cum)
            res["ap"][c, t] = voc_ap(recall, precision)
            lamr, fppi, mr = log_average_miss_rate(recall, fp_cum, B)
            res["lamr"][c, t] = lamr
            res["curves"][c, t] = {"recall": recall, "precision": precision, "fppi": fppi, "mr": mr}
    res["n_gt"] = np.array([sum(int((lab[:, 0].astype(np.int32) == c).sum()) for lab in labels) for c in range(nc)], dtype=np.int64)
    return res
