"""What the snowflake input transform costs on the device (dyk.functional.clahe / cutout: csrc/clahe.hip) beside two yardsticks
measured in the same process (GPU): dyk_image_prep on the same batch, and the HBM floor of 3 bytes per pixel.

Batch: two streams of uint8 [16,3,512,640] (96 planes of 327 680 pixels), the reference's CLAHE (clipLimit 1.0, 4 x 4 tiles of
160 x 128 pixels) and its 25 cut-outs of 16 x 16 per image.  Three inputs, seeded:
  noise      uniform over 0..255: every histogram bin gets about 80 of a tile's 20 480 pixels
  peaked     LWIR-like: a normal peak of sigma 2.5 grey levels plus 1 % hot pixels -- a few bins take nearly every LDS atomic
  constant   one value: the worst case, every atomic of a tile lands on one bin
Legs, alternating, `iters` back-to-back calls per leg and round, device events around them; median / min / max over `rounds`
after warm-up; each leg covers BOTH streams:
  clahe        2 x dyk_clahe (table launch + pixel launch each), tables and outputs allocated once
  cutout       2 x dyk_cutout_rects, rectangles already on the device
  image_prep   2 x dyk_image_prep uint8 -> fp32 at the same size (reads 1, writes 4 bytes per pixel)
  copy_u8      2 x a device copy of the uint8 batch (1 + 1 bytes per pixel)
`hbm`: a device copy of 2 x 1 GiB, timed the same way, gives the sustained bytes/s of this card; the floor of CLAHE is
3 bytes per pixel (the table pass reads the image, the pixel pass reads and writes it) over that rate.  The batch itself
(59 MB) fits the last-level cache, so a leg can run faster than that floor.
The host-side cv2 CLAHE this replaces cannot be timed here: no cv2 is installed where this project runs.
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/clahe_probe.py [--rounds 7] [--iters 20] [--out profiles/clahe.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, C, H, W = 16, 3, 512, 640
GRID, CLIP, N_SNOW, STEP = (4, 4), 1.0, 25, 16


def make_input(kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "noise":
        a = rng.randint(0, 256, size=(B, C, H, W))
    elif kind == "peaked":
        a = np.rint(rng.normal(92.0, 2.5, size=(B, C, H, W)))
        hot = rng.rand(B, C, H, W) < 0.01
        a[hot] = rng.randint(150, 256, size=int(hot.sum()))
    else:
        a = np.full((B, C, H, W), 92)
    return torch.from_numpy(np.clip(a, 0, 255).astype(np.uint8)).cuda()


def stat(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clahe_probe measures on the GPU; there is nothing to time without one")
    from dyk import functional as F
    from dyk.buildinfo import native_sha

    rng = np.random.RandomState(3)
    xy = rng.randint(0, H - 1, size=(B, N_SNOW, 2))
    rects = torch.from_numpy(np.concatenate([xy, np.minimum(xy + STEP - 1, H - 1)], 2).astype(np.int32)).cuda()
    pixels = 2 * B * C * H * W
    doc = {"code_sha": native_sha(), "device": torch.cuda.get_device_name(0), "batch": [2, B, C, H, W], "grid": list(GRID),
           "clip_limit": CLIP, "cutouts_per_image": N_SNOW, "pixels": pixels,
           "timed": "us per leg (both streams); device event time of %d back-to-back calls / %d; median [min, max] of %d rounds, "
                    "legs alternating" % (a.iters, a.iters, a.rounds), "inputs": {}}

    big_a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big_b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big_a.zero_()
    for _ in range(3):
        big_b.copy_(big_a)
    rates = [2.0 * (1 << 30) / (timed(lambda: big_b.copy_(big_a), 5) * 1e-6) for _ in range(a.rounds)]
    del big_a, big_b
    hbm = sorted(rates)[len(rates) // 2]
    doc["hbm"] = {"copy_bytes_per_s": stat(rates), "floor_bytes_per_pixel": 3, "clahe_floor_us": round(3.0 * pixels / hbm * 1e6, 2)}

    for kind in ("noise", "peaked", "constant"):
        v, l = make_input(kind, 1), make_input(kind, 2)
        ov, ol = torch.empty_like(v), torch.empty_like(l)
        cv, cl = v.clone(), l.clone()
        legs = {
            "clahe": lambda: (F.clahe(v, CLIP, GRID, out=ov), F.clahe(l, CLIP, GRID, out=ol)),
            "cutout": lambda: (F.cutout(cv, rects), F.cutout(cl, rects)),
            "image_prep": lambda: (F.prepare_images(v), F.prepare_images(l)),
            "copy_u8": lambda: (ov.copy_(v), ol.copy_(l)),
        }
        for fn in legs.values():                         # warm-up: code objects, allocator pools
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        first = F.clahe(v, CLIP, GRID).clone()
        us = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                us[k].append(timed(fn, a.iters))
        F.clahe(v, CLIP, GRID, out=ov)
        point = {"device_us": {k: stat(t) for k, t in us.items()}, "two_runs_equal": bool(torch.equal(first, ov))}
        med = point["device_us"]["clahe"]["median"]
        point["clahe_over_image_prep"] = round(med / point["device_us"]["image_prep"]["median"], 3)
        point["clahe_over_floor"] = round(med / doc["hbm"]["clahe_floor_us"], 3)
        point["clahe_pairs_per_s"] = round(B / (med * 1e-6), 1)
        doc["inputs"][kind] = point
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
