"""What the device resize / letterbox costs (dyk_resize_pad_pairs: csrc/letterbox.hip) beside two yardsticks measured in the same
process (GPU): dyk_image_prep on the same batch and the warp-only leg of dyk_augment_pairs on the same batch, and the HBM floor
of each configuration.

Batch: two streams of 16 images of 512 x 640 uint8, seeded noise, planar [16,3,512,640] and interleaved [16,512,640,3].  The
launch alone is timed -- the C entry with the records already on the device -- each figure covering BOTH streams:
  linear_chw / area_chw   0.8 x to 410 x 512 content at row 51 of 512 x 512 (the letterbox of a KAIST frame), planar sources
  linear_hwc / area_hwc   the same from interleaved BGR sources, channels reversed on the way
  pad_only                the frame copied to row 32 of 576 x 640
  area_2x                 exact 2 x AREA to 256 x 320
Beside them: image_prep (2 x dyk_image_prep uint8 -> fp32), augment_warp (dyk_augment_pairs with a 5 degree rotation, scale
0.9, nothing else: 512 x 640 output pixels per image against the 512 x 512 here), copy_u8 (a device copy of the batch).
Legs alternate; `iters` back-to-back calls per leg and round, device events around them; median / min / max over `rounds` after
warm-up.  `hbm`: a device copy of 2 x 1 GiB timed the same way gives the sustained bytes/s of this card; a configuration's
floor is (the source batch read once + the output written once) over that rate.  The batch (59 MB) fits the last-level cache,
so a leg can run faster than that floor.
`linear_not_slower_than_warp`: the one condition this kernel is held to (median against median of the same run).
`wrapper`: dyk.functional.resize_pad_pairs for linear_chw, host packing and the one record copy included (host clock around a
synchronise).
Not measured here, and said so: the host cv2 path this replaces (no cv2 where this project runs).
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/letterbox_probe.py [--rounds 9] [--iters 100] [--out profiles/letterbox.json]"""
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
        sys.exit("letterbox_probe measures on the GPU; there is nothing to time without one")
    from dyk import functional as F
    from dyk import lib as L
    from dyk.buildinfo import native_sha
    h = L.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    rng = np.random.RandomState(1)
    v = torch.from_numpy(rng.randint(0, 256, (B, C, H, W)).astype(np.uint8)).cuda()
    l = torch.from_numpy(rng.randint(0, 256, (B, C, H, W)).astype(np.uint8)).cuda()
    vh, lh = v.permute(0, 2, 3, 1).contiguous(), l.permute(0, 2, 3, 1).contiguous()
    keep = []

    def entry(srcs, geom, out_size, layout):
        Ho, Wo = out_size
        ov, ol = (torch.empty((B, C, Ho, Wo), dtype=torch.uint8, device="cuda") for _ in range(2))
        recs = (L.DykResizePadRec * B)()
        for b in range(B):
            recs[b] = L.DykResizePadRec(src_v=srcs[0][b].data_ptr(), src_l=srcs[1][b].data_ptr(), h=H, w=W, nh=geom[0], nw=geom[1], top=geom[2],
                                        left=geom[3], interp=geom[4])
        drecs = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).cuda()
        d = L.DykResizePadDesc(recs=drecs.data_ptr(), recs_host=ctypes.addressof(recs), dst_v=ov.data_ptr(), dst_l=ol.data_ptr(), B=B, Ho=Ho,
                               Wo=Wo, layout=layout, color=(ctypes.c_uint8 * 3)(114, 114, 114))
        keep.append((ov, ol, recs, drecs, d))

        def call():
            rc = h.dyk_resize_pad_pairs(ctypes.byref(d), stream())
            assert rc == 0, rc
        return call, (ov, ol)

    warp = torch.from_numpy(np.stack([F.invert_affine(rot(5, 0.9, W / 2, H / 2))] * B)).cuda()
    wv, wl = torch.empty_like(v), torch.empty_like(l)
    dw = L.DykAugmentDesc(src_v=v.data_ptr(), src_l=l.data_ptr(), dst_v=wv.data_ptr(), dst_l=wl.data_ptr(), N=B, B=B, H=H, W=W, Hc=H, Wc=W,
                          Ho=H, Wo=W, rects=None, minv=warp.data_ptr(), luts=None, flip=None)

    def augment_warp():
        rc = h.dyk_augment_pairs(ctypes.byref(dw), stream())
        assert rc == 0, rc

    cfg = {
        "linear_chw": ((v, l), (410, 512, 51, 0, 0), (512, 512), 0),
        "area_chw": ((v, l), (410, 512, 51, 0, 1), (512, 512), 0),
        "linear_hwc": ((vh, lh), (410, 512, 51, 0, 0), (512, 512), 1),
        "area_hwc": ((vh, lh), (410, 512, 51, 0, 1), (512, 512), 1),
        "pad_only": ((v, l), (512, 640, 32, 0, 0), (576, 640), 0),
        "area_2x": ((v, l), (256, 320, 0, 0, 1), (256, 320), 0),
    }
    legs, outs = {}, {}
    for k, c in cfg.items():
        legs[k], outs[k] = entry(*c)
    legs["image_prep"] = lambda: (F.prepare_images(v), F.prepare_images(l))
    legs["augment_warp"] = augment_warp
    legs["copy_u8"] = lambda: (wv.copy_(v), wl.copy_(l))
    px_in = 2 * B * C * H * W
    floors_bytes = {k: px_in + 2 * B * C * c[2][0] * c[2][1] for k, c in cfg.items()}
    floors_bytes["augment_warp"] = 2 * px_in

    doc = {"code_sha": native_sha(), "device": torch.cuda.get_device_name(0), "batch": [2, B, C, H, W],
           "legs": {k: {"content": list(c[1][:2]), "at": list(c[1][2:4]), "interp": ["LINEAR", "AREA"][c[1][4]], "out": list(c[2]),
                        "layout": ["chw", "hwc_bgr"][c[3]]} for k, c in cfg.items()},
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
    first = {k: (o[0].clone(), o[1].clone()) for k, o in outs.items()}
    us = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            us[k].append(timed(fn, a.iters))
    torch.cuda.synchronize()
    doc["device_us"] = {k: stat(t) for k, t in us.items()}
    doc["two_runs_equal"] = all(torch.equal(first[k][0], o[0]) and torch.equal(first[k][1], o[1]) for k, o in outs.items())
    doc["hwc_equals_chw"] = bool(torch.equal(outs["linear_hwc"][0], outs["linear_chw"][0].flip(1)) and
                                 torch.equal(outs["area_hwc"][1], outs["area_chw"][1].flip(1)))
    med = lambda k: doc["device_us"][k]["median"]
    doc["over_floor"] = {k: round(med(k) / doc["hbm"]["floor_us"][k], 2) for k in floors_bytes}
    doc["over_image_prep"] = {k: round(med(k) / med("image_prep"), 2) for k in cfg}
    doc["over_augment_warp"] = {k: round(med(k) / med("augment_warp"), 2) for k in cfg}
    doc["linear_not_slower_than_warp"] = bool(med("linear_chw") <= med("augment_warp"))
    doc["pairs_per_s"] = {k: round(B / (med(k) * 1e-6), 1) for k in cfg}

    # the public wrapper: host packing + one pinned copy + launch, host clock around a synchronise
    geom = [(410, 512, 51, 0, 0)] * B
    ov, ol = outs["linear_chw"]
    for _ in range(3):
        F.resize_pad_pairs(v, l, geom, (512, 512), color=(114, 114, 114), out=(ov, ol))
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(20):
            F.resize_pad_pairs(v, l, geom, (512, 512), color=(114, 114, 114), out=(ov, ol))
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6 / 20)
    doc["wrapper"] = {"config": "linear_chw", "host_us_per_call": stat(wall)}
    doc["not_measured"] = ["the host cv2 path of the reference loader (cv2.resize, copyMakeBorder; no cv2 here)"]
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
