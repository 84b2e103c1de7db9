"""What the per-batch step of the evaluator costs (dyk.evalmap.DetectionEvaluator.update: one dyk_eval_match launch) beside
the host loop it replaces, in ONE process (GPU).

Inputs, seeded: the padded NMS output [16, 100, 6] of one evaluation batch with about 60 (50..70) or exactly 100 detections
per image, 4..20 ground-truth boxes per image in 640 x 512 frames letterboxed into 512 x 416, nc = 1 and 80, 1 and 10 IoU
thresholds.  Detections are jittered copies of ground truth plus clutter in descending score.

Legs, alternating, `iters` back-to-back calls per leg and round, median / min / max over `rounds` after warm-up:
  update_a, update_b  DetectionEvaluator.update((out, counts), targets, shapes, img1_shape, ratio_pad, targets_host=...): the
                      table upload and the launch.  Two equal legs: their difference is the spread of the measurement.
  update_sync         the same without targets_host: `targets` is copied back to count the ground truth (one blocking copy)
  host_loop           the loop of evaluate.py:76-106 / `_ap5` of tests/test_eval_ap.py on the same detections: per image a
                      scale_coords launch, the device-to-host copies of boxes, scores and classes, a dict per detection
Each leg is timed twice in the same pass: device events around the `iters` calls (what the stream was busy or kept waiting),
and the host clock around the calls plus a final synchronise (what the caller waits).  The records are not cleared between
rounds: the arrays grow geometrically during warm-up.
Then one `compute()` over 5000 batches' worth of records (5000 x 100 detections): the device-to-host copy and compute_map,
host clock, median of 3.
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/evalmap_probe.py [--rounds 7] [--iters 20] [--out profiles/evalmap.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, MAX_NUM, W0, H0, IMG1 = 16, 100, 640, 512, (416, 512)
RATIO_PAD = ((0.8, 0.8), (0.0, 3.2))


def make_batch(nc, per_image, seed):
    """(out [B, MAX_NUM, 6] on the network input, counts, targets [nt, 6]) -- per_image: (lo, hi) detections per image"""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, MAX_NUM, 6), np.float32)
    counts, tg = [], []
    for b in range(B):
        k = int(rng.integers(4, 21))
        bw, bh = rng.uniform(12, 80, k), rng.uniform(24, 160, k)
        xc, yc = rng.uniform(bw / 2, W0 - bw / 2), rng.uniform(bh / 2, H0 - bh / 2)
        cls = rng.integers(0, nc, k)
        tg += [[b, cls[j], xc[j] / W0, yc[j] / H0, bw[j] / W0, bh[j] / H0] for j in range(k)]
        n = int(rng.integers(per_image[0], per_image[1] + 1))
        j = rng.integers(0, k, n)
        jit = rng.uniform(-0.2, 0.2, (n, 4)) * np.stack([bw[j], bh[j], bw[j], bh[j]], 1)
        box = np.stack([xc[j] - bw[j] / 2, yc[j] - bh[j] / 2, xc[j] + bw[j] / 2, yc[j] + bh[j] / 2], 1) + jit
        clutter = rng.random(n) < 0.3
        box[clutter] = np.stack([rng.uniform(0, W0 - 50, n), rng.uniform(0, H0 - 50, n)] * 2, 1)[clutter] + [0, 0, 30, 45]
        d = np.zeros((n, 6), np.float32)
        d[:, :4] = box * RATIO_PAD[0][0] + [RATIO_PAD[1][0], RATIO_PAD[1][1]] * 2
        d[:, 4] = np.sort(rng.uniform(0.05, 1.0, n))[::-1]
        d[:, 5] = np.where(rng.random(n) < 0.9, cls[j], rng.integers(0, nc, n))
        out[b, :n] = d
        counts.append(n)
    return out, counts, np.array(tg, np.float32)


def host_loop(dets, scale_coords):
    """evaluate.py:76-106 as `_ap5` of tests/test_eval_ap.py restates it, with the class column a multi-class caller needs"""
    preds = []
    for idx, p in enumerate(dets):
        if p is None:
            continue
        boxes = scale_coords(IMG1, p[:, :4].clone(), (H0, W0), RATIO_PAD)
        boxes, conf, cls = boxes.cpu().numpy(), p[:, 4].cpu().numpy(), p[:, 5].cpu().numpy()
        preds += [{"img_id": idx, "conf": float(conf[i]), "cls": int(cls[i]), "bbox": boxes[i]} for i in range(boxes.shape[0])]
    return preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--compute-batches", type=int, default=5000 // B + 1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "evalmap_probe.py measures on the GPU; there is nothing to time without one"
    from build_utils.utils import scale_coords
    from code_sha import code_sha
    from dyk.evalmap import DetectionEvaluator
    shapes = [(W0, H0)] * B
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "B": B, "max_num": MAX_NUM,
           "timed": "us per call; device = event time of %d back-to-back calls / %d, wall = host clock around them and a final "
                    "synchronise / %d; median [min, max] of %d rounds, legs alternating" % (a.iters, a.iters, a.iters, a.rounds),
           "points": {}, "compute": {}}
    for nc in (1, 80):
        for T in (1, 10):
            thr = tuple(round(0.5 + 0.05 * i, 2) for i in range(T))
            for tag, per_image in (("about60", (50, 70)), ("exactly100", (100, 100))):
                out_h, counts, tg_h = make_batch(nc, per_image, 1000 + nc)
                out, tg = torch.from_numpy(out_h).cuda(), torch.from_numpy(tg_h).cuda()
                tg_host = torch.from_numpy(tg_h)
                dets = [out[b, :n] for b, n in enumerate(counts)]
                ev = DetectionEvaluator(nc, thr)
                legs = [("update_a", lambda: ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)),
                        ("update_b", lambda: ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)),
                        ("update_sync", lambda: ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD)),
                        ("host_loop", lambda: host_loop(dets, scale_coords))]
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
                stat = lambda v: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                med = lambda d, leg: float(np.median(d[leg]))
                doc["points"]["nc%d_T%d_%s" % (nc, T, tag)] = {
                    "detections": int(sum(counts)), "targets": int(tg_h.shape[0]),
                    "device_us": {leg: stat(v) for leg, v in dev_us.items()}, "wall_us": {leg: stat(v) for leg, v in wall_us.items()},
                    "equal_legs_spread_us": {"device": round(abs(med(dev_us, "update_a") - med(dev_us, "update_b")), 1),
                                             "wall": round(abs(med(wall_us, "update_a") - med(wall_us, "update_b")), 1)},
                    "host_loop_over_update_wall": round(med(wall_us, "host_loop") / med(wall_us, "update_a"), 2)}
                if tag == "exactly100" and (nc, T) in ((1, 1), (80, 10)):
                    ev.reset()
                    for _ in range(a.compute_batches):
                        ev.update((out, counts), tg, shapes, IMG1, RATIO_PAD, targets_host=tg_host)
                    torch.cuda.synchronize()
                    ms = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        res = ev.compute()
                        ms.append((time.perf_counter() - t0) * 1e3)
                    doc["compute"]["nc%d_T%d" % (nc, T)] = {"records": int(ev.records()["conf"].shape[0]), "images": ev.num_imgs,
                                                            "ms": stat(ms), "map": res["map"]}
                del ev
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
