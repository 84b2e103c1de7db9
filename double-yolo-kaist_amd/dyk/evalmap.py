"""Multi-class detection evaluators: per-batch matching on the device, once-per-epoch curve arithmetic in numpy.

`DetectionEvaluator` -- per-class AP at one or several IoU thresholds, LAMR and mAP under the VOC / KAIST rule.
The per-batch half runs on the device (dyk_eval_match, csrc/evalmap.hip): one launch per evaluation batch matches every
detection the NMS kept to the ground truth of its image and class and appends one record per detection to device arrays
this object owns.  The once-per-epoch half -- sorting, cumulative sums, `voc_ap`, `log_average_miss_rate` -- is the numpy
code of other_utils.metrics (`compute_map`), fed by one device-to-host copy in `compute()`.

    ev = DetectionEvaluator(nc, iou_thresholds=(0.5,))
    for imgs, targets, shapes in loader:                       # replaces evaluate.py:76-117
        out, counts = non_max_suppression(model(imgs)[0], conf, iou, return_padded=True)
        ev.update((out, counts), targets, shapes, img1_shape=imgs.shape[2:])
    res = ev.compute()                                         # res["map50"], res["ap"][c, t], res["summary"]

The matching rule is the VOC / KAIST one of `compute_ap_lamr`, applied per class (see `compute_map` for what that means
next to pycocotools); with nc = 1, one threshold 0.5 and ground truth in every image the result is compute_ap_lamr's.

`CocoEvaluator` -- the COCO protocol the training harness validates with (train_utils/kaist_train_eval_utils.py:122-190):
score-ordered best-unclaimed matching at ten IoU thresholds in four area ranges, maxDets 1 / 10 / 100, 101-point
interpolated precision, and the twelve `stats`.  Same `update()` / `compute()` shape; the device half is
dyk_eval_match_coco (csrc/evalmap_coco.hip, the protocol is stated in include/dyk_hip.h), the host half
other_utils.metrics.coco_accumulate.

    ev = CocoEvaluator(nc)
    for imgs, targets, shapes in loader:                       # replaces kaist_train_eval_utils.py:122-190
        ev.update(non_max_suppression(model(imgs)[0], conf, iou), targets, shapes, img1_shape=imgs.shape[2:])
    stats = ev.compute()["stats"]                              # what train.py consumes: stats[0] mAP@[.5:.95], stats[1] mAP@.5

No COCO tool is installed where this project runs: the protocol is implemented from the published algorithm and held to
tests/coco_ref.py and its hand-worked cases; agreement with pycocotools itself is derived, not measured.
"""
import ctypes

import numpy as np
import torch

from . import lib as L
from .lib import check, load


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _RecordStore:
    """What the two evaluators share: the growing per-detection record arrays on the device, the input forms of `update`,
    its checks, and the one table (counts, rec_off, gt_off, shape0, unpad) a launch reads."""
    _FIELDS = ()
    _ENTRY = ""

    def _reset_store(self):
        self._rec = None            # field -> device array of capacity self._cap
        self._cap = 0
        self._err = None            # [2] int32 on the device: the kernel's error words, set and never cleared by it
        self._n = 0                 # records appended
        self._gt_base = 0           # rows of `targets` seen before this batch: `match` is made global with it in records()
        self._bases = []            # (first record, record count, target-row base) per update
        self.num_imgs = 0

    def _reserve(self, need, dev):
        if self._rec is not None and need <= self._cap:
            return
        cap = max(1024, self._cap)
        while cap < need:
            cap *= 2
        rec = {k: torch.empty((cap,) + tail, dtype=dt, device=dev) for k, dt, tail in self._FIELDS}
        if self._rec is not None:
            for k in rec:
                rec[k][:self._n].copy_(self._rec[k][:self._n])
        else:
            self._err = torch.zeros(2, dtype=torch.int32, device=dev)
        self._rec, self._cap = rec, cap

    @staticmethod
    def _padded(dets):
        """(out [B, max_num, 6], counts) of either form `update` takes"""
        if isinstance(dets, tuple):
            out, counts = dets
            return out, [max(int(c), 0) for c in counts]
        counts = [0 if d is None else int(d.shape[0]) for d in dets]
        some = [d for d in dets if d is not None]
        if not some:
            return None, counts
        base = some[0]._base
        if base is not None and base.dim() == 3 and base.shape[0] == len(dets) and base.is_contiguous() and all(
                d._base is base and d.data_ptr() == base[b].data_ptr() for b, d in enumerate(dets) if d is not None):
            return base, counts                     # the list non_max_suppression returns: views of its padded output
        out = some[0].new_zeros((len(dets), max(counts), 6), dtype=torch.float32)
        for b, d in enumerate(dets):
            if d is not None:
                out[b, :counts[b]] = d
        return out, counts

    def _inputs(self, dets, targets, shapes, targets_host):
        """the checks of `update` that touch nothing: (out, counts, host targets [nt,6], boxes per image, classes)"""
        me = type(self).__name__
        out, counts = self._padded(dets)
        for t, what in ((out, "detections"), (targets, "targets")):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise L.DykError("%s.update runs on the MI355X HIP path only (%s: got a %s); there is no CPU "
                                 "fallback" % (me, what, "%s tensor" % t.device.type if isinstance(t, torch.Tensor) else type(t).__name__))
        B = len(counts)
        if len(shapes) != B:
            raise ValueError("%s.update: %d images of detections, %d shapes" % (me, B, len(shapes)))
        th = (targets if targets_host is None else targets_host).detach().cpu().numpy().reshape(-1, 6)
        nt = th.shape[0]
        img = th[:, 0].astype(np.int64)
        if nt and (np.any(np.diff(img) < 0) or img[0] < 0 or img[-1] >= B):
            raise ValueError("%s.update: targets must be sorted by their image column, all in [0, %d)" % (me, B))
        per_img = np.bincount(img, minlength=B)
        if nt and per_img.max() > L.EVAL_MAX_GT:
            raise ValueError("%s.update: image %d of the batch has %d ground-truth boxes, the limit is %d "
                             "(DYK_EVAL_MAX_GT)" % (me, int(per_img.argmax()), int(per_img.max()), L.EVAL_MAX_GT))
        gcls = th[:, 1].astype(np.int64)
        if nt and (gcls.min() < 0 or gcls.max() >= self.nc):
            raise ValueError("%s.update: a ground-truth class outside [0, %d)" % (me, self.nc))
        return out, counts, th, per_img, gcls

    def _check_out(self, out, counts):
        me, B = type(self).__name__, len(counts)
        if out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != B or out.shape[2] != 6 or not out.is_contiguous():
            raise L.DykError("%s.update expects the fp32 [B, max_num, 6] output of non_max_suppression, got %s %s"
                             % (me, out.dtype, tuple(out.shape)))
        if max(counts) > out.shape[1]:
            raise ValueError("%s.update: a count of %d detections in a [%d, %d, 6] output" % ((me, max(counts)) + tuple(out.shape[:2])))

    def _tables(self, counts, per_img, shapes, img1_shape, ratio_pad, dev):
        """every table of the launch in one host array, one host-to-device copy: counts, rec_off, gt_off, shape0, unpad"""
        B = len(counts)
        tab = np.zeros(9 * B + 1, dtype=np.int32)
        tab[0:B] = counts
        tab[B:2 * B] = self._n + np.concatenate(([0], np.cumsum(counts)[:-1]))
        tab[2 * B:3 * B + 1] = np.concatenate(([0], np.cumsum(per_img)))
        tab[3 * B + 1:5 * B + 1] = np.asarray([(int(w), int(h)) for w, h in shapes], dtype=np.int32).reshape(-1)
        if img1_shape is not None:
            unpad = tab[5 * B + 1:].view(np.float32).reshape(B, 4)
            rps = ratio_pad if isinstance(ratio_pad, list) else [ratio_pad] * B
            for b, ((w0, h0), rp) in enumerate(zip(shapes, rps)):
                if rp is not None:
                    gain, pad = rp[0][0], rp[1]
                else:                              # scale_coords (build_utils/utils.py), img0_shape = (h0, w0)
                    gain = max(img1_shape) / max(h0, w0)
                    pad = ((img1_shape[1] - w0 * gain) / 2, (img1_shape[0] - h0 * gain) / 2)
                if float(np.float32(gain)) == 0.0:
                    raise ValueError("%s.update: image %d has a zero letterbox gain" % (type(self).__name__, b))
                unpad[b] = (pad[0], pad[1], gain, 1.0)
        return torch.from_numpy(tab).to(dev, non_blocking=True)

    def _fill_inputs(self, d, out, tab_d, targets, nt, B, img1_shape):
        """the input fields the two descriptors have in common; returns what must stay alive until the launch is issued"""
        tg = targets.detach()
        if tg.dtype != torch.float32 or not tg.is_contiguous():
            tg = tg.to(torch.float32).contiguous()
        p = tab_d.data_ptr()
        d.out, d.counts, d.rec_off, d.gt_off, d.shape0 = out.data_ptr(), p, p + 4 * B, p + 8 * B, p + 4 * (3 * B + 1)
        d.unpad = p + 4 * (5 * B + 1) if img1_shape is not None else None
        d.targets = tg.data_ptr() if nt else None
        for t, v in enumerate(self.iou_thresholds):
            d.thr[t] = v
        d.B, d.max_num, d.nt, d.nc, d.T, d.rec_cap = B, int(out.shape[1]), nt, self.nc, len(self.iou_thresholds), self._cap
        return tg

    def _raise_on_flags(self, err):
        if err[0]:
            raise ValueError("%s: a detection's class index lies outside [0, %d) (%s error flag)" % (type(self).__name__, self.nc, self._ENTRY))
        if err[1]:
            raise L.DykError("%s refused an image's table entries (records, target rows or box count out of range)" % self._ENTRY)

    def summary(self):
        return self.compute()["summary"]


class DetectionEvaluator(_RecordStore):
    _FIELDS = (("conf", torch.float32, ()), ("cls", torch.int32, ()), ("tp_mask", torch.int32, ()),
               ("match", torch.int32, ()), ("iou", torch.float64, ()), ("box", torch.float32, (4,)))
    _ENTRY = "dyk_eval_match"

    def __init__(self, nc, iou_thresholds=(0.5,), names=None):
        self.nc = int(nc)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        if self.nc < 1:
            raise ValueError("DetectionEvaluator(nc=...) must be at least 1, got %r" % (nc,))
        if not 1 <= len(self.iou_thresholds) <= L.EVAL_MAX_THR:
            raise ValueError("DetectionEvaluator takes 1 to %d IoU thresholds (DYK_EVAL_MAX_THR), got %d"
                             % (L.EVAL_MAX_THR, len(self.iou_thresholds)))
        self.names = names
        self.reset()

    def reset(self):
        self._reset_store()
        self.n_gt = np.zeros(self.nc, dtype=np.int64)

    # ------------------------------------------------------------------------------------------------------------
    def update(self, dets, targets, shapes, img1_shape=None, ratio_pad=None, targets_host=None):
        """One evaluation batch.

        dets: what non_max_suppression returns -- the list of [n,6] device tensors or None, or the pair (out, counts) of
        return_padded=True.  targets: the batch's [nt,6] device tensor (image in batch, class, xc, yc, w, h; relative),
        sorted by image as the collate function leaves it.  shapes: per image the original (width, height).
        img1_shape (h, w) of the network input switches the un-letterbox transform of scale_coords on; ratio_pad as for
        scale_coords: one ((ratio_h, ratio_w), (pad_x, pad_y)) for the batch, or a list with one per image.  Without
        img1_shape the boxes are taken as they are.

        One launch, no device synchronisation.  The ground truth is counted per class on the host: from `targets_host`,
        the loader's host copy of the same tensor, when it is given; otherwise `targets` is copied back, which waits for
        that one copy (non_max_suppression has just drained the stream)."""
        out, counts, th, per_img, gcls = self._inputs(dets, targets, shapes, targets_host)
        B, nt = len(counts), th.shape[0]
        self.n_gt += np.bincount(gcls, minlength=self.nc)
        self.num_imgs += B
        total = sum(counts)
        if total == 0:
            self._gt_base += nt
            return
        self._check_out(out, counts)
        self._reserve(self._n + total, out.device)
        tab_d = self._tables(counts, per_img, shapes, img1_shape, ratio_pad, out.device)
        d = L.DykEvalMatchDesc()
        tg = self._fill_inputs(d, out, tab_d, targets, nt, B, img1_shape)
        r = self._rec
        d.conf, d.cls, d.tp_mask, d.match = r["conf"].data_ptr(), r["cls"].data_ptr(), r["tp_mask"].data_ptr(), r["match"].data_ptr()
        d.iou, d.box, d.err = r["iou"].data_ptr(), r["box"].data_ptr(), self._err.data_ptr()
        check(load().dyk_eval_match(ctypes.byref(d), _stream()), "dyk_eval_match")
        del tg
        self._bases.append((self._n, total, self._gt_base))
        self._n += total
        self._gt_base += nt

    # ------------------------------------------------------------------------------------------------------------
    def compute(self):
        """One device-to-host copy of conf, cls and tp_mask (and the launch error words), then
        other_utils.metrics.compute_map on them.  ValueError when a detection's class was outside [0, nc)."""
        from other_utils.metrics import compute_map
        n = self._n
        if n:
            r = self._rec
            head = torch.cat([r["conf"][:n].view(torch.int32), r["cls"][:n], r["tp_mask"][:n], self._err]).cpu().numpy()
            self._raise_on_flags(head[3 * n:])
            conf, cls, tp = head[:n].view(np.float32), head[n:2 * n], head[2 * n:3 * n].view(np.uint32)
        else:
            conf, cls, tp = np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
        return compute_map(conf, cls, tp, self.n_gt, self.num_imgs, self.iou_thresholds, names=self.names)

    def records(self):
        """every record array as numpy, for inspection: conf, cls, tp_mask (uint32), match (row of the targets of ALL
        updates laid end to end, or -1), iou (fp64), box [n,4]"""
        n = self._n
        if not n:
            return {"conf": np.zeros(0, np.float32), "cls": np.zeros(0, np.int32), "tp_mask": np.zeros(0, np.uint32),
                    "match": np.zeros(0, np.int32), "iou": np.zeros(0, np.float64), "box": np.zeros((0, 4), np.float32)}
        rec = {k: v[:n].cpu().numpy() for k, v in self._rec.items()}
        rec["tp_mask"] = rec["tp_mask"].view(np.uint32)
        for first, count, base in self._bases:
            m = rec["match"][first:first + count]
            m[m >= 0] += base
        return rec


class CocoEvaluator(_RecordStore):
    """COCO-protocol bbox evaluation: `update()` per batch (one dyk_eval_match_coco launch, no synchronisation),
    `compute()` once (one device-to-host copy, then other_utils.metrics.coco_accumulate).  `compute()["stats"]` is the list
    of twelve numbers the training harness returns (COCOeval.stats).  Defaults: thresholds np.linspace(.5, .95, 10), area
    ranges all / small / medium / large, max_dets (1, 10, 100), boxes rounded half-to-even as the harness rounds them."""
    _ENTRY = "dyk_eval_match_coco"

    def __init__(self, nc, iou_thresholds=None, area_ranges=None, max_dets=(1, 10, 100), round_boxes=True, names=None):
        from other_utils.metrics import COCO_AREA_RANGES, COCO_IOU_THRESHOLDS
        self.nc = int(nc)
        self.iou_thresholds = tuple(float(t) for t in (COCO_IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds))
        self.area_ranges = tuple((float(lo), float(hi)) for lo, hi in (COCO_AREA_RANGES if area_ranges is None else area_ranges))
        self.max_dets = tuple(int(m) for m in max_dets)
        self.round_boxes = bool(round_boxes)
        T, A = len(self.iou_thresholds), len(self.area_ranges)
        if self.nc < 1:
            raise ValueError("CocoEvaluator(nc=...) must be at least 1, got %r" % (nc,))
        if not 1 <= T <= L.EVAL_MAX_THR:
            raise ValueError("CocoEvaluator takes 1 to %d IoU thresholds (DYK_EVAL_MAX_THR), got %d" % (L.EVAL_MAX_THR, T))
        if not 1 <= A <= L.EVAL_MAX_AREA:
            raise ValueError("CocoEvaluator takes 1 to %d area ranges (DYK_EVAL_MAX_AREA), got %d" % (L.EVAL_MAX_AREA, A))
        if A * T > 64:
            raise ValueError("CocoEvaluator: %d area ranges x %d thresholds = %d pairs, the limit is 64 (one lane decides one pair)"
                             % (A, T, A * T))
        if not self.max_dets or min(self.max_dets) < 1 or list(self.max_dets) != sorted(set(self.max_dets)):
            raise ValueError("CocoEvaluator: max_dets must be ascending positive integers, got %r" % (max_dets,))
        self._FIELDS = (("conf", torch.float32, ()), ("cls", torch.int32, ()), ("img", torch.int32, ()), ("rank", torch.int32, ()),
                        ("box", torch.float32, (4,)), ("darea", torch.float64, ()), ("dtm", torch.int32, (A,)),
                        ("dtig", torch.int32, (A,)), ("match", torch.int16, (A, T)))
        self.names = names
        self.reset()

    def reset(self):
        self._reset_store()
        self._row0 = []             # per update: for every record the first `targets` row (of all updates) of its image
        self.n_gt_ka = np.zeros((self.nc, len(self.area_ranges)), dtype=np.int64)    # non-ignored boxes per class and area range

    def count_ground_truth(self, targets, shapes):
        """[nc, A] non-ignored boxes per class and area range of one batch's host `targets` [nt,6] (numpy): the kernel's
        fp32 arithmetic (include/dyk_hip.h) in numpy.  `update` adds this to n_gt_ka."""
        th = np.asarray(targets).reshape(-1, 6)
        gcls = th[:, 1].astype(np.int64)
        out = np.zeros_like(self.n_gt_ka)
        if th.shape[0]:
            wh0 = np.asarray([(w, h) for w, h in shapes], dtype=np.float32)[th[:, 0].astype(np.int64)]
            t32 = th.astype(np.float32)
            gw, gh = t32[:, 4] * wh0[:, 0], t32[:, 5] * wh0[:, 1]
            garea = gw.astype(np.float64) * gh.astype(np.float64)
            for a, (lo, hi) in enumerate(self.area_ranges):
                out[:, a] = np.bincount(gcls[~((garea < lo) | (garea > hi))], minlength=self.nc)
        return out

    def update(self, dets, targets, shapes, img1_shape=None, ratio_pad=None, targets_host=None):
        """One evaluation batch; the arguments of DetectionEvaluator.update.  One launch, no device synchronisation."""
        out, counts, th, per_img, gcls = self._inputs(dets, targets, shapes, targets_host)
        B, nt = len(counts), th.shape[0]
        total = sum(counts)
        if total:
            self._check_out(out, counts)
            if out.shape[1] > L.EVAL_COCO_MAX_NUM:
                raise ValueError("CocoEvaluator.update: %d detection rows per image, the limit is %d (DYK_EVAL_COCO_MAX_NUM)"
                                 % (out.shape[1], L.EVAL_COCO_MAX_NUM))
        self.n_gt_ka += self.count_ground_truth(th, shapes)
        img_base = self.num_imgs
        self.num_imgs += B
        if total == 0:
            self._gt_base += nt
            return
        self._reserve(self._n + total, out.device)
        tab_d = self._tables(counts, per_img, shapes, img1_shape, ratio_pad, out.device)
        d = L.DykEvalCocoDesc()
        tg = self._fill_inputs(d, out, tab_d, targets, nt, B, img1_shape)
        for k, _, _ in self._FIELDS:
            setattr(d, k, self._rec[k].data_ptr())
        d.err = self._err.data_ptr()
        for a, (lo, hi) in enumerate(self.area_ranges):
            d.area[a][0], d.area[a][1] = lo, hi
        d.A, d.max_det, d.round_boxes, d.img_base = len(self.area_ranges), max(self.max_dets), int(self.round_boxes), img_base
        check(load().dyk_eval_match_coco(ctypes.byref(d), _stream()), "dyk_eval_match_coco")
        del tg
        self._bases.append((self._n, total, self._gt_base))
        # the kernel's `match` counts within the image's own rows: the first row of each record's image, for records()
        self._row0.append(np.repeat(self._gt_base + np.concatenate(([0], np.cumsum(per_img)[:-1])), counts))
        self._n += total
        self._gt_base += nt

    def compute(self):
        """One device-to-host copy of conf, cls, img, rank, dtm and dtig (and the launch error words), then
        other_utils.metrics.coco_accumulate.  ValueError when a detection's class was outside [0, nc)."""
        from other_utils.metrics import coco_accumulate
        n, A = self._n, len(self.area_ranges)
        if n:
            r = self._rec
            head = torch.cat([r["conf"][:n].view(torch.int32), r["cls"][:n], r["img"][:n], r["rank"][:n],
                              r["dtm"][:n].reshape(-1), r["dtig"][:n].reshape(-1), self._err]).cpu().numpy()
            self._raise_on_flags(head[(4 + 2 * A) * n:])
            conf, cls, img, rank = head[:n].view(np.float32), head[n:2 * n], head[2 * n:3 * n], head[3 * n:4 * n]
            dtm = head[4 * n:(4 + A) * n].view(np.uint32).reshape(n, A)
            dtig = head[(4 + A) * n:(4 + 2 * A) * n].view(np.uint32).reshape(n, A)
        else:
            conf, cls, img, rank = np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
            dtm, dtig = np.zeros((0, A), np.uint32), np.zeros((0, A), np.uint32)
        return coco_accumulate(conf, cls, img, rank, dtm, dtig, self.n_gt_ka, self.iou_thresholds, self.area_ranges,
                               self.max_dets, names=self.names)

    def records(self):
        """every record array as numpy, for inspection: conf, cls, img, rank, box [n,4], darea (fp64), dtm / dtig [n,A]
        (uint32, bit t), match [n,A,T] (int32: row of the targets of ALL updates laid end to end, or -1)"""
        n, A, T = self._n, len(self.area_ranges), len(self.iou_thresholds)
        if not n:
            return {"conf": np.zeros(0, np.float32), "cls": np.zeros(0, np.int32), "img": np.zeros(0, np.int32),
                    "rank": np.zeros(0, np.int32), "box": np.zeros((0, 4), np.float32), "darea": np.zeros(0, np.float64),
                    "dtm": np.zeros((0, A), np.uint32), "dtig": np.zeros((0, A), np.uint32), "match": np.zeros((0, A, T), np.int32)}
        rec = {k: v[:n].cpu().numpy() for k, v in self._rec.items()}
        rec["dtm"], rec["dtig"] = rec["dtm"].view(np.uint32), rec["dtig"].view(np.uint32)
        m = rec["match"].astype(np.int32)
        rec["match"] = np.where(m >= 0, m + np.concatenate(self._row0).astype(np.int32)[:, None, None], -1)
        return rec
