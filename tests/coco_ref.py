"""The yardstick of the COCO-protocol evaluator (dyk_eval_match_coco + other_utils.metrics.coco_accumulate): a deliberately
plain restatement of the protocol in include/dyk_hip.h with Python loops, one (image, class, area, threshold) at a time.
It shares no code with the kernel's host side or with coco_accumulate, and nothing with any COCO tool: it is written from
the published description of the algorithm.  Python floats are IEEE doubles and numpy float32 scalars stay float32, so every
step rounds as the protocol says.

Inputs: dets   per image a float32 [n,6] array (x1, y1, x2, y2 in the ORIGINAL frame -- un-letterboxed and clipped, not yet
               rounded --, conf, cls) in NMS order, or None
        labels per image a float32 [k,5] array (cls, xc, yc, w, h; relative)
        shapes per image (width, height)

`evaluate` returns the record fields of CocoEvaluator.records() (match indexes the rows of all labels laid end to end),
`npig` [K, A], `precision` [T, 101, K, A, M], `recall` [T, K, A, M], the twelve `stats`, and `counters`: how often each
rule of the protocol decided something, so that a case set that stops exercising a rule can be noticed."""
import numpy as np

F = np.float32
THRESHOLDS = tuple(float(v) for v in np.linspace(0.5, 0.95, 10))
AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
MAX_DETS = (1, 10, 100)


def ground_truth(lab, w0, h0):
    """[(class, gx, gy, gw, gh, garea)] of one image: fp32 steps, then doubles"""
    out = []
    for row in np.asarray(lab, dtype=F).reshape(-1, 5):
        xc, yc, w, h = row[1], row[2], row[3], row[4]
        gx = (xc - F(0.5) * w) * F(w0)
        gy = (yc - F(0.5) * h) * F(h0)
        gw = w * F(w0)
        gh = h * F(h0)
        out.append((int(row[0]), float(gx), float(gy), float(gw), float(gh), float(gw) * float(gh)))
    return out


def iou_of(dx, dy, dw, dh, darea, gx, gy, gw, gh, garea):
    a, b = dx + dw, gx + gw
    lo = dx if dx > gx else gx
    w = (a if a < b else b) - lo
    if w <= 0:
        return 0.0
    a, b = dy + dh, gy + gh
    lo = dy if dy > gy else gy
    h = (a if a < b else b) - lo
    if h <= 0:
        return 0.0
    i = w * h
    return i / (darea + garea - i)


def outside(area, rng):
    return area < rng[0] or area > rng[1]


def evaluate(dets, labels, shapes, nc, thresholds=THRESHOLDS, areas=AREAS, max_dets=MAX_DETS, round_boxes=True):
    B, T, A, M = len(labels), len(thresholds), len(areas), len(max_dets)
    assert len(dets) == B == len(shapes)
    max_det = max(max_dets)
    first = [0]
    row0 = [0]
    for d, lab in zip(dets, labels):
        first.append(first[-1] + (0 if d is None else d.shape[0]))
        row0.append(row0[-1] + lab.shape[0])
    n = first[-1]
    rec = {"conf": np.zeros(n, F), "cls": np.zeros(n, np.int32), "img": np.zeros(n, np.int32), "rank": np.zeros(n, np.int32),
           "box": np.zeros((n, 4), F), "darea": np.zeros(n, np.float64), "dtm": np.zeros((n, A), np.uint32),
           "dtig": np.zeros((n, A), np.uint32), "match": np.full((n, A, T), -1, np.int16)}
    local = np.full((n, A, T), -1, np.int64)                     # `match` before the rows of earlier images are added
    npig = np.zeros((nc, A), np.int64)
    cnt = {"gt_ignored": [0] * A, "gt_kept": [0] * A, "matched_to_ignored": 0, "unmatched_ignored": 0, "not_argmax": 0,
           "stopped_before_better_ignored": 0, "rank_cut": 0, "iou_ties": 0}

    for b in range(B):
        w0, h0 = shapes[b]
        gts = ground_truth(labels[b], w0, h0)
        for g in gts:
            for a in range(A):
                if outside(g[5], areas[a]):
                    cnt["gt_ignored"][a] += 1
                else:
                    cnt["gt_kept"][a] += 1
                    npig[g[0], a] += 1
        d = dets[b]
        if d is None:
            continue
        nd = d.shape[0]
        boxes = np.asarray(d[:, :4], dtype=F)
        if round_boxes:
            boxes = np.rint(boxes)                               # half to even, float32
        geo = []
        for i in range(nd):
            x1, y1, x2, y2 = boxes[i]
            dw, dh = x2 - x1, y2 - y1                            # float32
            geo.append((float(x1), float(y1), float(dw), float(dh), float(dw) * float(dh)))
            r = first[b] + i
            rec["conf"][r], rec["cls"][r], rec["img"][r] = d[i, 4], int(d[i, 5]), b
            rec["box"][r], rec["darea"][r] = boxes[i], geo[i][4]
        classes = sorted(set(int(c) for c in d[:, 5]))
        for c in classes:
            mine = [i for i in range(nd) if int(d[i, 5]) == c]
            ranked = sorted(mine, key=lambda i: -float(d[i, 4]))          # Python's sort is stable: equal scores keep NMS order
            for rank, i in enumerate(ranked):
                rec["rank"][first[b] + i] = rank
                if rank >= max_det:
                    cnt["rank_cut"] += 1
            if c < 0 or c >= nc:
                continue
            ranked = ranked[:max_det]
            rows = [k for k, g in enumerate(gts) if g[0] == c]
            iou = [[iou_of(*geo[i], *gts[k][1:]) for k in rows] for i in ranked]
            for a in range(A):
                ign = [outside(gts[k][5], areas[a]) for k in rows]
                visit = [j for j in range(len(rows)) if not ign[j]] + [j for j in range(len(rows)) if ign[j]]
                for t in range(T):
                    taken = [False] * len(rows)
                    for q, i in enumerate(ranked):
                        row = iou[q]
                        best = min(thresholds[t], 1 - 1e-10)
                        m = -1
                        for j in visit:
                            if m >= 0 and not ign[m] and ign[j]:
                                break
                            v = row[j]
                            if v < best:
                                continue
                            if taken[j]:
                                continue
                            if m >= 0 and v == best:
                                cnt["iou_ties"] += 1
                            best, m = v, j
                        r = first[b] + i
                        if m >= 0:
                            taken[m] = True
                            rec["dtm"][r, a] |= np.uint32(1 << t)
                            local[r, a, t] = rows[m]
                            if row[m] < max(row):
                                cnt["not_argmax"] += 1
                            if ign[m]:
                                rec["dtig"][r, a] |= np.uint32(1 << t)
                                cnt["matched_to_ignored"] += 1
                            elif any(ign[j] and not taken[j] and row[j] > row[m] for j in range(len(rows))):
                                cnt["stopped_before_better_ignored"] += 1
                        elif outside(geo[i][4], areas[a]):
                            rec["dtig"][r, a] |= np.uint32(1 << t)
                            cnt["unmatched_ignored"] += 1
    rec["match"] = local.astype(np.int16)                        # as the kernel writes it: a row of the image's own labels

    res = accumulate(rec, npig, thresholds, areas, max_dets)
    res["records"], res["npig"], res["counters"] = rec, npig, cnt
    res["match_global"] = _global_match(local, first, row0)
    return res


def _global_match(local, first, row0):
    """records()["match"] of the evaluator: rows of the labels of all images laid end to end"""
    out = np.full(local.shape, -1, np.int32)
    for b in range(len(first) - 1):
        s = slice(first[b], first[b + 1])
        out[s] = np.where(local[s] >= 0, local[s] + row0[b], -1)
    return out


def accumulate(rec, npig, thresholds, areas, max_dets):
    T, A, M, K = len(thresholds), len(areas), len(max_dets), npig.shape[0]
    grid = np.linspace(0.0, 1.0, 101)
    precision = -np.ones((T, 101, K, A, M))
    recall = -np.ones((T, K, A, M))
    n = rec["conf"].shape[0]
    for k in range(K):
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for mi, mx in enumerate(max_dets):
                # image order, then rank order; then a stable sort by descending score
                sel = [r for r in range(n) if rec["cls"][r] == k and rec["rank"][r] < mx]
                sel.sort(key=lambda r: (int(rec["img"][r]), int(rec["rank"][r])))
                sel.sort(key=lambda r: -float(rec["conf"][r]))
                for t in range(T):
                    tp = fp = 0.0
                    rc, pr = [], []
                    for r in sel:
                        matched = (int(rec["dtm"][r, a]) >> t) & 1
                        ignored = (int(rec["dtig"][r, a]) >> t) & 1
                        if not ignored:
                            if matched:
                                tp += 1.0
                            else:
                                fp += 1.0
                        rc.append(tp / float(npig[k, a]))
                        pr.append(tp / (fp + tp + np.spacing(1)))
                    recall[t, k, a, mi] = rc[-1] if sel else 0.0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    j = 0
                    for gi, g in enumerate(grid):
                        while j < len(rc) and rc[j] < g:          # the first index with rc >= g
                            j += 1
                        precision[t, gi, k, a, mi] = pr[j] if j < len(rc) else 0.0
    return {"precision": precision, "recall": recall, "stats": stats_of(precision, recall, thresholds, len(areas), len(max_dets))}


def _mean(cells):
    vals = [float(v) for v in np.asarray(cells).reshape(-1) if v > -1]
    return sum(vals) / len(vals) if vals else -1.0


def stats_of(precision, recall, thresholds, A, M):
    """the twelve numbers; area ranges 1..3 are small / medium / large when they exist, the last max_dets entry stands for
    "100", entries 0..2 for the three AR lines; what does not exist is -1"""
    def t_of(v):
        hits = [t for t, x in enumerate(thresholds) if float(x) == v]
        return hits[0] if hits else None

    def ap(t=None, a=0):
        if a >= A:
            return -1.0
        p = precision[:, :, :, a, M - 1] if t is None else precision[t, :, :, a, M - 1]
        return _mean(p)

    def ar(a=0, m=None):
        m = M - 1 if m is None else m
        if a >= A or m >= M:
            return -1.0
        return _mean(recall[:, :, a, m])

    t50, t75 = t_of(0.5), t_of(0.75)
    return [ap(), ap(t50) if t50 is not None else -1.0, ap(t75) if t75 is not None else -1.0, ap(a=1), ap(a=2), ap(a=3),
            ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3)]
