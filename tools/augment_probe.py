"""What the device augmentation costs (dyk_augment_pairs: csrc/augment.hip) beside two yardsticks measured in the same process
(GPU): dyk_image_prep and dyk_clahe on the same batch, and the HBM floor of each configuration.

Batch: two streams of uint8 [16,3,512,640], seeded noise.  The launch alone is timed -- the C entry with the per-image
parameters already on the device -- in four configurations, each covering BOTH streams:
  jitter     HSV tables only, out of place
  warp       5 degree rotation about the centre, scale 0.9, nothing else
  mosaic     four-image canvas of 1280 x 1280 -> 640 x 640 with a random_affine matrix (border -320), tables and flip
  all_on     plain image: warp + tables + flip
Beside them: image_prep (2 x dyk_image_prep uint8 -> fp32), clahe (2 x dyk_clahe, 4 x 4 tiles), copy_u8 (a device copy of the
batch).  Legs alternate; `iters` back-to-back calls per leg and round, device events around them; median / min / max over
`rounds` after warm-up.  `hbm`: a device copy of 2 x 1 GiB timed the same way gives the sustained bytes/s of this card; a
configuration's floor is (bytes it must read once + bytes it writes once) over that rate, where the bytes read are taken as
the whole source batch (for the mosaic: as many bytes as the output has, if that is less).  The batch (59 MB) fits the
last-level cache, so a leg can run faster than that floor.
`rows`: the all_on and the jitter configuration with 1, 2 (the built-in choice), 4, 8 and 16 output rows per workgroup through
dyk_augment_pairs_rows, alternating in the same run.
`wrapper`: dyk.functional.augment_pairs for all_on, host packing and the one parameter copy included (host clock around a
synchronise).
Not measured here, and said so: the host cv2 path this replaces (no cv2 where this project runs), and what drawing the mosaic
companions from the batch does to AP.
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/augment_probe.py [--rounds 9] [--iters 100] [--out profiles/augment.json]"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, C, H, W = 16, 3, 512, 640
S = 640                                       # mosaic: img_size


def rot(deg, scale, cx, cy):
    a = deg * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy], [0, 0, 1]])


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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_probe measures on the GPU; there is nothing to time without one")
    import random
    from build_utils import augment as A
    from dyk import functional as F
    from dyk import lib as L
    from dyk.buildinfo import native_sha
    h = L.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    rng = np.random.RandomState(1)
    v = torch.from_numpy(rng.randint(0, 256, (B, C, H, W)).astype(np.uint8)).cuda()
    l = torch.from_numpy(rng.randint(0, 256, (B, C, H, W)).astype(np.uint8)).cuda()
    random.seed(2)
    np.random.seed(2)
    luts = np.stack([A._hsv_tables(0.0138, 0.678, 0.36) for _ in range(B)])
    flips = (np.arange(B) % 2).astype(np.uint8)
    warp = np.stack([F.invert_affine(rot(5, 0.9, W / 2, H / 2))] * B)
    mos_r, mos_m = [], []
    for b in range(B):
        r, _ = A._draw_mosaic(b, B, S, [(H, W)] * B, [np.zeros((0, 5))] * B)
        M, _ = A._draw_matrix(2 * S, 2 * S, 5, 0.05, 0.1, 2, -S // 2)
        mos_r.append(r)
        mos_m.append(F.invert_affine(M))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_luts, d_flip, d_warp, d_mr, d_mm = dev(luts), dev(flips), dev(warp), dev(np.stack(mos_r)), dev(np.array(mos_m))
    ov, ol = torch.empty_like(v), torch.empty_like(l)
    mv, ml = (torch.empty((B, C, S, S), dtype=torch.uint8, device="cuda") for _ in range(2))

    def entry(dst, Ho, Wo, rects=None, canvas=(H, W), minv=None, luts=None, flip=None):
        p = lambda t: None if t is None else t.data_ptr()
        d = L.DykAugmentDesc(src_v=v.data_ptr(), src_l=l.data_ptr(), dst_v=dst[0].data_ptr(), dst_l=dst[1].data_ptr(), N=B, B=B, H=H, W=W,
                             Hc=canvas[0], Wc=canvas[1], Ho=Ho, Wo=Wo, rects=p(rects), minv=p(minv), luts=p(luts), flip=p(flip))

        def call(rows=None):
            rc = h.dyk_augment_pairs(ctypes.byref(d), stream()) if rows is None else h.dyk_augment_pairs_rows(ctypes.byref(d), rows, stream())
            assert rc == 0, rc
        return call

    legs = {
        "jitter": entry((ov, ol), H, W, luts=d_luts),
        "warp": entry((ov, ol), H, W, minv=d_warp),
        "mosaic": entry((mv, ml), S, S, rects=d_mr, canvas=(2 * S, 2 * S), minv=d_mm, luts=d_luts, flip=d_flip),
        "all_on": entry((ov, ol), H, W, minv=d_warp, luts=d_luts, flip=d_flip),
        "image_prep": lambda: (F.prepare_images(v), F.prepare_images(l)),
        "clahe": lambda: (F.clahe(v, 1.0, (4, 4), out=ov), F.clahe(l, 1.0, (4, 4), out=ol)),
        "copy_u8": lambda: (ov.copy_(v), ol.copy_(l)),
    }
    px_in, px_full, px_mos = 2 * B * C * H * W, 2 * B * C * H * W, 2 * B * C * S * S
    # bytes read once + written once (see the module text)
    floors_bytes = {"jitter": px_in + px_full, "warp": px_in + px_full, "all_on": px_in + px_full, "mosaic": min(px_in, px_mos) + px_mos}

    doc = {"code_sha": native_sha(), "device": torch.cuda.get_device_name(0), "batch": [2, B, C, H, W], "mosaic": {"canvas": [2 * S, 2 * S], "out": [S, S]},
           "timed": "us per leg (both streams); device event time of %d back-to-back calls / %d; median [min, max] of %d rounds, legs "
                    "alternating" % (a.iters, a.iters, a.rounds)}
    big_a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big_b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    big_a.zero_()
    for _ in range(3):
        big_b.copy_(big_a)
    rates = [2.0 * (1 << 30) / (timed(lambda: big_b.copy_(big_a), 5) * 1e-6) for _ in range(a.rounds)]
    del big_a, big_b
    hbm = sorted(rates)[len(rates) // 2]
    doc["hbm"] = {"copy_bytes_per_s": stat(rates), "floor_us": {k: round(n / hbm * 1e6, 2) for k, n in floors_bytes.items()}}

    for fn in legs.values():                             # warm-up: code objects, allocator pools
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    legs["all_on"]()
    first = (ov.clone(), ol.clone())
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, a.iters))
    legs["all_on"]()
    torch.cuda.synchronize()
    doc["device_us"] = {k: stat(t) for k, t in us.items()}
    doc["two_runs_equal"] = bool(torch.equal(first[0], ov) and torch.equal(first[1], ol))
    doc["over_floor"] = {k: round(doc["device_us"][k]["median"] / doc["hbm"]["floor_us"][k], 2) for k in floors_bytes}
    doc["over_image_prep"] = {k: round(doc["device_us"][k]["median"] / doc["device_us"]["image_prep"]["median"], 2) for k in floors_bytes}
    doc["pairs_per_s"] = {k: round(B / (doc["device_us"][k]["median"] * 1e-6), 1) for k in floors_bytes}

    # rows per workgroup, alternating in the same run
    rows_us = {k: {r: [] for r in (1, 2, 4, 8, 16)} for k in ("all_on", "jitter")}
    for _ in range(a.rounds):
        for k, per in rows_us.items():
            for r in per:
                legs[k](r)
                per[r].append(timed(lambda: legs[k](r), a.iters))
    doc["rows"] = {k: {str(r): stat(t) for r, t in per.items()} for k, per in rows_us.items()}

    # the public wrapper: host packing + one pinned copy + launch, host clock around a synchronise
    Mf = np.stack([rot(5, 0.9, W / 2, H / 2)[:2]] * B)
    for _ in range(3):
        F.augment_pairs(v, l, matrices=Mf, luts=luts, flip=flips, out=(ov, ol))
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(20):
            F.augment_pairs(v, l, matrices=Mf, luts=luts, flip=flips, out=(ov, ol))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6 / 20)
    doc["wrapper"] = {"config": "all_on", "host_us_per_call": stat(wall)}
    doc["not_measured"] = ["the host cv2 path of the reference loader (no cv2 here)", "the AP effect of drawing mosaic companions from the batch"]
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
