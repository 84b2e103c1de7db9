"""What the row-wise multi-label NMS (dyk_nms_rows) costs beside the per-pair pass it replaces (dyk_nms with multi_label = 1),
in ONE process (GPU).

Inputs, seeded (`make_pred`): [16, 20160, 5 + nc] for nc = 2, 20, 80.  Boxes: 25 clusters per image, centres uniform in a
512 x 640 image, w in 16..76, h in 32..152, jitter N(0, (4, 4, 3, 6)).  obj = u^3 and every class score = u with u uniform in
[0, 1): most rows are far below any threshold, as after a sigmoid head.  For each shape three thresholds are found by bisection
on the CPU so that the mean candidate count per image is about 300, about 5000, and 1.25 x the default capacity max(N, 8192) (so
every image overflows it).

Legs, alternating, `iters` back-to-back calls between two device events, median / min / max over `rounds` after warm-up:
  pairs    dyk_nms, multi_label = 1, preallocated per-pair workspace (the parent's path, still in the library)
  rows     dyk_nms_rows, preallocated workspace of the default capacity (at the third threshold it ends after the count, -1)
  wrapper  dyk.detect.non_max_suppression end to end: allocations, launch(es), the host sync on `counts`, per-image slicing; at
           the third threshold that is the row-wise launch, the sync, and the per-pair call behind it
At every timed point the outputs of `pairs` and `rows` (where the batch fits) and of `pairs` and `wrapper` (always) are asserted
bit-identical.  Workspace bytes of each leg are recorded.  Prints one JSON document; `--out FILE` also writes it.
usage: python tools/nms_rows_probe.py [--rounds 7] [--iters 10] [--out profiles/nms_rows.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, N, IOU, MAX_NUM = 16, 20160, 0.6, 100


def make_pred(nc, seed):
    g = torch.Generator().manual_seed(seed)
    ncl = 25
    cx = torch.rand(B, ncl, generator=g) * 560 + 40
    cy = torch.rand(B, ncl, generator=g) * 430 + 40
    w = torch.rand(B, ncl, generator=g) * 60 + 16
    h = torch.rand(B, ncl, generator=g) * 120 + 32
    which = torch.randint(0, ncl, (B, N), generator=g)
    jit = torch.randn(B, N, 4, generator=g) * torch.tensor([4.0, 4.0, 3.0, 6.0])
    p = torch.zeros(B, N, 5 + nc)
    p[..., 0] = torch.gather(cx, 1, which) + jit[..., 0]
    p[..., 1] = torch.gather(cy, 1, which) + jit[..., 1]
    p[..., 2] = (torch.gather(w, 1, which) + jit[..., 2]).clamp(min=3.0)
    p[..., 3] = (torch.gather(h, 1, which) + jit[..., 3]).clamp(min=3.0)
    p[..., 4] = torch.rand(B, N, generator=g) ** 3
    p[..., 5:] = torch.rand(B, N, nc, generator=g)
    return p


def counts_at(p, t):
    """(alive rows, candidates) per image at threshold t (fp32, strict, as the kernels decide)"""
    t = float(np.float32(t))
    alive = p[..., 4] > t
    ok = ((p[..., 5:] * p[..., 4:5]) > t) & alive[..., None]
    return alive.sum(1), ok.sum((1, 2))


def threshold_for(p, target):
    lo, hi = 0.0, 1.0                                 # candidates fall as t rises
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if float(counts_at(p, mid)[1].float().mean()) > target:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


class Direct:
    """preallocated buffers and descriptor of one entry"""

    def __init__(self, L, pred, conf, rows_cap):
        h = L.load()
        no = pred.shape[2]
        self.rows = rows_cap is not None
        self.per = int(h.dyk_nms_rows_workspace_bytes(N, rows_cap)) if self.rows else int(h.dyk_nms_workspace_bytes(N, no, 1))
        self.ws = torch.empty(B * self.per, dtype=torch.uint8, device="cuda")
        self.out = torch.zeros((B, MAX_NUM, 6), device="cuda")
        self.out_rows = torch.zeros((B, MAX_NUM), dtype=torch.int32, device="cuda")
        self.counts = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.n_cand = torch.zeros(B, dtype=torch.int32, device="cuda")
        d = self.d = L.DykNmsRowsDesc() if self.rows else L.DykNmsDesc()
        d.pred, d.out, d.out_rows, d.counts, d.ws, d.ws_per_image = (pred.data_ptr(), self.out.data_ptr(), self.out_rows.data_ptr(),
                                                                     self.counts.data_ptr(), self.ws.data_ptr(), self.per)
        d.B, d.N, d.no, d.conf_thres, d.iou_thres = B, N, no, conf, IOU
        d.multi_label, d.agnostic, d.max_num, d.n_classes = 1, 0, MAX_NUM, 0
        if self.rows:
            d.cand_cap, d.n_cand = rows_cap, self.n_cand.data_ptr()
        self.fn = h.dyk_nms_rows if self.rows else h.dyk_nms

    def run(self):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.fn(ctypes.byref(self.d), 0, s) if self.rows else self.fn(ctypes.byref(self.d), s)
        assert rc == 0, rc

    def result(self):
        cnt = self.counts.cpu().tolist()
        return cnt, [self.out[b, :max(n, 0)].cpu().numpy().view(np.uint32) for b, n in enumerate(cnt)], \
            [self.out_rows[b, :max(n, 0)].cpu().numpy() for b, n in enumerate(cnt)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", type=int, nargs="*", default=[2, 20, 80])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from code_sha import code_sha
    from dyk import detect, lib as L
    cap = detect.nms_default_candidates(N)
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "iou_thres": IOU, "max_num": MAX_NUM,
           "default_capacity": cap, "NMS_ROWS_MIN_NC": detect.NMS_ROWS_MIN_NC,
           "inputs": "make_pred(nc, seed = 900 + nc) of tools/nms_rows_probe.py: clustered boxes, obj = u^3, class scores = u",
           "timed": "us per call = device-event time of %d back-to-back calls / %d; median [min, max] of %d rounds, legs alternating; "
                    "the wrapper leg includes its allocations and its host sync" % (a.iters, a.iters, a.rounds),
           "shapes": {}}
    for nc in a.classes:
        p = make_pred(nc, 900 + nc)
        dev = p.cuda().contiguous()
        points = {}
        for tag, target in (("n300", 300), ("n5000", 5000), ("overflow", 1.25 * cap)):
            conf = threshold_for(p, target)
            alive, n = counts_at(p, conf)
            fits = int(n.max()) <= cap
            assert fits == (tag != "overflow") and (fits or int(n.min()) > cap), (nc, tag, n.tolist())
            pairs, rows = Direct(L, dev, conf, None), Direct(L, dev, conf, cap)

            def wrapper():
                return detect.non_max_suppression(dev, conf_thres=conf, iou_thres=IOU, multi_label=True, max_num=MAX_NUM, return_rows=True)

            legs = [("pairs", pairs.run), ("rows", rows.run), ("wrapper", wrapper)]
            for _ in range(a.warmup):
                for _, fn in legs:
                    fn()
            torch.cuda.synchronize()
            # the check: same bits from the old and the new route at this point
            c0 = detect.nms_route_counts()
            pc, po, pr = pairs.result()
            rc_, ro, rr = rows.result()
            wres, wrows = wrapper()
            c1 = detect.nms_route_counts()
            assert rows.n_cand.cpu().tolist() == n.tolist(), (nc, tag)
            if fits:
                assert rc_ == pc and all(np.array_equal(x, y) for x, y in zip(ro, po)) and all(np.array_equal(x, y) for x, y in zip(rr, pr))
            else:
                assert rc_ == [-1] * B
            routed = nc >= detect.NMS_ROWS_MIN_NC                          # below it the wrapper keeps the per-pair call
            assert c1["rows"] - c0["rows"] == int(routed) and c1["rows_overflow"] - c0["rows_overflow"] == int(routed and not fits)
            for b in range(B):
                wb = np.zeros((0, 6), np.uint32) if wres[b] is None else wres[b].cpu().numpy().view(np.uint32)
                assert np.array_equal(wb, po[b]), (nc, tag, b)
                assert (wrows[b] is None and pc[b] == 0) or np.array_equal(wrows[b].cpu().numpy(), pr[b]), (nc, tag, b)
            us = {leg: [] for leg, _ in legs}
            for _ in range(a.rounds):
                for leg, fn in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    us[leg].append(e0.elapsed_time(e1) * 1e3 / a.iters)
            med = {leg: float(np.median(v)) for leg, v in us.items()}
            spread = {leg: float(max(v) - min(v)) for leg, v in us.items()}
            points[tag] = {"conf_thres": conf, "alive_rows_per_image": [int(alive.min()), int(alive.max())],
                           "candidates_per_image": [int(n.min()), int(n.max())], "kept_per_image": sorted(set(pc)),
                           "fits_default_capacity": fits, "outputs_bit_identical": True,
                           "us_per_call": {leg: {"median": round(med[leg], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                           for leg, v in us.items()},
                           "rows_minus_pairs_us": round(med["rows"] - med["pairs"], 1),
                           "spread_us": round(max(spread["rows"], spread["pairs"]), 1),
                           "wrapper_minus_pairs_us": round(med["wrapper"] - med["pairs"], 1)}
            del pairs, rows
        h = L.load()
        doc["shapes"]["[%d, %d, %d]" % (B, N, 5 + nc)] = {
            "workspace_bytes": {"pairs": B * int(h.dyk_nms_workspace_bytes(N, 5 + nc, 1)), "rows": B * int(h.dyk_nms_rows_workspace_bytes(N, cap)),
                                "wrapper": "rows when the batch fits; rows, then pairs after it, when an image overflows"},
            "points": points}
        del dev
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
