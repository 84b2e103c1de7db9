"""What the per-batch step of the COCO-protocol evaluator costs (dyk.evalmap.CocoEvaluator.update: one dyk_eval_match_coco
launch) beside the VOC-rule evaluator's step and beside the host yardstick, in ONE process (GPU).

Inputs, seeded (make_batch of tools/evalmap_probe.py): the padded NMS output [16, 100, 6] of one evaluation batch with 90..100
kept detections per image (what is left of about 300 raw candidates), 4..20 ground-truth boxes per image in 640 x 512 frames
letterboxed into 512 x 416, nc = 1 and 80; the protocol's defaults (ten thresholds, four area ranges, max_dets 1 / 10 / 100).

Legs, alternating, `iters` back-to-back calls per leg and round, median / min / max over `rounds` after warm-up:
  coco_update_a, _b   CocoEvaluator.update((out, counts), targets, shapes, img1_shape, ratio_pad, targets_host=...): the
                      ground-truth count, the table upload and the launch.  Two equal legs: their difference is the spread.
  coco_launch         dyk_eval_match_coco alone, on a descriptor built once
  voc_update          DetectionEvaluator.update with ten thresholds on the same batch (the path that existed before)
  voc_launch          dyk_eval_match alone
Each leg is timed twice in the same pass: device events around the `iters` calls, and the host clock around the calls plus a
final synchronise.  `worst_image`: the launch alone on the worst image the limits admit -- 1024 boxes of one class, 100
detections, every detection a jittered copy of a box -- in the same alternation with coco_launch of the nc = 1 batch.
`host_ref_ms`: tests/coco_ref.evaluate on the batch (matching and accumulation in plain Python), host clock, median of 3.
Then one `compute()` over about 500 000 records: the device-to-host copy and coco_accumulate, host clock, median of 3.
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/evalmap_coco_probe.py [--rounds 7] [--iters 20] [--out profiles/evalmap_coco.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from evalmap_probe import B, H0, IMG1, MAX_NUM, RATIO_PAD, W0, make_batch  # noqa: E402


def worst_image(seed=7):
    """(out [1, 100, 6], counts, targets [1024, 6]): 1024 boxes of class 0, 100 detections on a hundred of them"""
    rng = np.random.default_rng(seed)
    k = 1024
    side, asp = np.exp(rng.uniform(np.log(8), np.log(220), k)), np.exp(rng.uniform(-0.5, 0.5, k))
    bw, bh = np.minimum(side * asp, W0), np.minimum(side / asp, H0)
    xc, yc = rng.uniform(bw / 2, W0 - bw / 2), rng.uniform(bh / 2, H0 - bh / 2)
    tg = np.stack([np.zeros(k), np.zeros(k), xc / W0, yc / H0, bw / W0, bh / H0], 1).astype(np.float32)
    j = rng.permutation(k)[:100]
    box = np.stack([xc[j] - bw[j] / 2, yc[j] - bh[j] / 2, xc[j] + bw[j] / 2, yc[j] + bh[j] / 2], 1)
    box += rng.uniform(-0.1, 0.1, (100, 4)) * np.stack([bw[j], bh[j], bw[j], bh[j]], 1)
    out = np.zeros((1, 100, 6), np.float32)
    out[0, :, :4] = box * RATIO_PAD[0][0] + [RATIO_PAD[1][0], RATIO_PAD[1][1]] * 2
    out[0, :, 4] = np.sort(rng.uniform(0.05, 1.0, 100))[::-1]
    return out, [100], tg


class Launch:
    """one dyk_eval_match_coco / dyk_eval_match launch on a descriptor built once; every array is kept alive here"""

    def __init__(self, coco, out_h, counts, tg_h, nc, thr, areas):
        from dyk import lib as L
        nb, T, A = len(counts), len(thr), len(areas or ())
        n = int(sum(counts))
        i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32).cuda()
        per_img = np.bincount(tg_h[:, 0].astype(np.int64), minlength=nb)
        k = self.keep = {"out": torch.from_numpy(out_h).cuda(), "counts": i32(counts), "rec_off": i32(np.concatenate(([0], np.cumsum(counts)[:-1]))),
                         "targets": torch.from_numpy(tg_h).cuda(), "gt_off": i32(np.concatenate(([0], np.cumsum(per_img)))),
                         "shape0": i32([(W0, H0)] * nb), "unpad": torch.tensor([[RATIO_PAD[1][0], RATIO_PAD[1][1], RATIO_PAD[0][0], 1.0]] * nb).cuda(),
                         "err": torch.zeros(2, dtype=torch.int32).cuda(), "conf": torch.empty(n).cuda(), "cls": i32(np.zeros(n)),
                         "box": torch.empty(n, 4).cuda()}
        if coco:
            k.update(img=i32(np.zeros(n)), rank=i32(np.zeros(n)), darea=torch.empty(n, dtype=torch.float64).cuda(),
                     dtm=i32(np.zeros((n, A))), dtig=i32(np.zeros((n, A))), match=torch.empty((n, A, T), dtype=torch.int16).cuda())
            d = L.DykEvalCocoDesc()
            for a, (lo, hi) in enumerate(areas):
                d.area[a][0], d.area[a][1] = lo, hi
            d.A, d.max_det, d.round_boxes, d.img_base = A, 100, 1, 0
            self.fn = L.load().dyk_eval_match_coco
        else:
            k.update(tp_mask=i32(np.zeros(n)), match=i32(np.zeros(n)), iou=torch.empty(n, dtype=torch.float64).cuda())
            d = L.DykEvalMatchDesc()
            self.fn = L.load().dyk_eval_match
        for name, v in k.items():
            setattr(d, name, v.data_ptr())
        for t, v in enumerate(thr):
            d.thr[t] = v
        d.B, d.max_num, d.nt, d.nc, d.T, d.rec_cap = nb, out_h.shape[1], tg_h.shape[0], nc, T, n
        self.d = d

    def __call__(self):
        rc = self.fn(ctypes.byref(self.d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def measure(legs, a):
    for _ in range(a.warmup):
        for _, fn in legs:
            for _ in range(a.iters):
                fn()
    torch.cuda.synchronize()
    dev_us, wall_us = {leg: [] for leg, _ in legs}, {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            wall_us[leg].append((time.perf_counter() - t0) * 1e6 / a.iters)
            dev_us[leg].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return {"device_us": {leg: stat(v) for leg, v in dev_us.items()}, "wall_us": {leg: stat(v) for leg, v in wall_us.items()}}


def stat(v):
    return {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compute-batches", type=int, default=500000 // (B * MAX_NUM) + 1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "evalmap_coco_probe.py measures on the GPU; there is nothing to time without one"
    import coco_ref
    from build_utils.utils import clip_coords, scale_coords
    from code_sha import code_sha
    from dyk.evalmap import CocoEvaluator, DetectionEvaluator
    from other_utils.metrics import COCO_AREA_RANGES, COCO_IOU_THRESHOLDS
    shapes = [(W0, H0)] * B
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "B": B, "max_num": MAX_NUM,
           "timed": "us per call; device = event time of %d back-to-back calls / %d, wall = host clock around them and a final "
                    "synchronise / %d; median [min, max] of %d rounds, legs alternating" % (a.iters, a.iters, a.iters, a.rounds),
           "points": {}, "compute": {}}
    launches = {}
    for nc in (1, 80):
        out_h, counts, tg_h = make_batch(nc, (90, 100), 1000 + nc)
        out, tg, tg_host = torch.from_numpy(out_h).cuda(), torch.from_numpy(tg_h).cuda(), torch.from_numpy(tg_h)
        ev, voc = CocoEvaluator(nc), DetectionEvaluator(nc, COCO_IOU_THRESHOLDS)
        coco_launch = launches[nc] = Launch(True, out_h, counts, tg_h, nc, COCO_IOU_THRESHOLDS, COCO_AREA_RANGES)
        voc_launch = Launch(False, out_h, counts, tg_h, nc, COCO_IOU_THRESHOLDS, None)
        legs = [("coco_update_a", lambda: ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)),
                ("coco_update_b", lambda: ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)),
                ("coco_launch", coco_launch), ("voc_update", lambda: voc.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)),
                ("voc_launch", voc_launch)]
        point = measure(legs, a)
        point.update(detections=int(sum(counts)), targets=int(tg_h.shape[0]))
        # the host yardstick on the same batch: original-frame boxes as the device makes them, then plain Python
        back = []
        for b, n in enumerate(counts):
            boxes = scale_coords(IMG1, out[b, :n, :4].clone(), (H0, W0), RATIO_PAD)
            clip_coords(boxes, (H0, W0))
            back.append(np.concatenate([boxes.cpu().numpy(), out_h[b, :n, 4:]], 1))
        labels = [tg_h[tg_h[:, 0] == b][:, 1:] for b in range(B)]
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = coco_ref.evaluate(back, labels, shapes, nc)
            ms.append((time.perf_counter() - t0) * 1e3)
        point["host_ref_ms"] = stat(ms)
        ev.reset()
        ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)
        point["stats_equal_host_ref"] = bool(np.abs(np.array(ev.compute()["stats"]) - np.array(ref["stats"])).max() <= 1e-10)
        doc["points"]["nc%d" % nc] = point
        ev.reset()
        for _ in range(a.compute_batches):
            ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = ev.compute()
            ms.append((time.perf_counter() - t0) * 1e3)
        doc["compute"]["nc%d" % nc] = {"records": int(ev._n), "images": ev.num_imgs, "ms": stat(ms), "stats": [round(s, 6) for s in res["stats"]]}
        del ev, voc
    out_h, counts, tg_h = worst_image()
    worst = Launch(True, out_h, counts, tg_h, 1, COCO_IOU_THRESHOLDS, COCO_AREA_RANGES)
    doc["worst_image"] = measure([("worst_image_launch", worst), ("coco_launch_nc1_batch", launches[1])], a)
    doc["worst_image"].update(boxes=1024, detections=100, classes=1)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
