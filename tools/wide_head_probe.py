"""Cost of detection heads wider than 32 channels -> profiles/wide_heads.json.

1. dyk_head_decode (one launch: y -> p and the decoded rows of io) against the two launches it replaces in a wide eval plan
   (dyk_head_permute_fwd, dyk_yolo_decode), on the three head maps of the target cfg at 640 x 512, batch 16, classes = 20 and 80.
   Both legs run interleaved in rounds; a sample is the mean of a batch of back-to-back launches between two events; median,
   min, max and the spread over the samples are recorded, and the achieved bytes per second of the fused kernel (y read once, p
   and the io rows written) beside what the bandwidth-bound kernels of profiles/tensor_stats.json reach.
2. The target cfg with classes=80 / filters=255 (generated here, not shipped) beside classes=1 in the same run: train-step ms,
   eval pairs per second, one non_max_suppression call with multi_label off / on and its workspace bytes.

    python tools/wide_head_probe.py [--quick]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "double-yolo-kaist_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

TARGET = "kaist_dyolov4_fshare_global_concat_se3"
ANCHORS = [1.25, 1.625, 2.0, 3.75, 4.125, 2.875]


def _stats(samples):
    s = sorted(samples)
    med = statistics.median(s)
    return {"n": len(s), "median_us": round(med, 3), "min_us": round(s[0], 3), "max_us": round(s[-1], 3),
            "mean_us": round(sum(s) / len(s), 3), "spread": round((s[-1] - s[0]) / med, 4)}


def _timed(fn, batch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(batch):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / batch


def kernel_points(rounds, samples, batch):
    from dyk import lib as L, ops
    from dyk.plan import head_ld
    h = L.load()
    out = []
    B, na = 16, 3
    for nc in (20, 80):
        no = 5 + nc
        ld = head_ld(na * no)
        for stride in (8, 16, 32):
            ny, nx = 512 // stride, 640 // stride
            rows = na * ny * nx
            y = torch.randn(B, ny, nx, ld, device="cuda") * 2.0
            p = torch.empty(B, na, ny, nx, no, device="cuda")
            io = torch.empty(B, rows + 5, no, device="cuda")
            p2, io2 = torch.empty_like(p), torch.empty_like(io)
            st = ops._stream()
            f, d = L.DykHeadDecodeDesc(), L.DykDecodeDesc()
            for q, dst_p, dst_io in ((f, p, io), (d, p2, io2)):
                q.p, q.io = dst_p.data_ptr(), dst_io.data_ptr()
                q.B, q.na, q.ny, q.nx, q.no = B, na, ny, nx, no
                q.rows_total, q.row_offset, q.v4, q.stride = rows + 5, 5, 1, float(stride)
                for k, v in enumerate(ANCHORS):
                    q.anchor_vec[k] = v
            f.y, f.ld = y.data_ptr(), ld

            def fused():
                h.dyk_head_decode(ctypes.byref(f), st)

            def two():
                h.dyk_head_permute_fwd(y.data_ptr(), p2.data_ptr(), B, ny, nx, na, no, ld, st)
                h.dyk_yolo_decode(ctypes.byref(d), st)

            for fn in (fused, two):                          # warm-up: code objects loaded, clocks up
                _timed(fn, 50)
            assert torch.equal(p, p2) and torch.equal(io[:, 5:].view(torch.int32), io2[:, 5:].view(torch.int32))
            t = {"fused": [], "two_launch": []}
            for _ in range(rounds):
                for name, fn in (("fused", fused), ("two_launch", two)):
                    for _ in range(samples):
                        t[name].append(_timed(fn, batch))
            elems = B * rows * no
            fused_bytes = B * ny * nx * na * no * 4 + 2 * elems * 4       # the channels read of y + p + io rows
            rec = {"nc": nc, "no": no, "ld": ld, "map": [ny, nx], "batch": B, "elements": elems,
                   "fused": _stats(t["fused"]), "two_launch": _stats(t["two_launch"]), "fused_bytes": fused_bytes}
            rec["fused_over_two_launch"] = round(rec["fused"]["median_us"] / rec["two_launch"]["median_us"], 4)
            rec["fused_GB_per_s"] = round(fused_bytes / rec["fused"]["median_us"] / 1e3, 1)
            rec["fused_not_slower"] = rec["fused"]["median_us"] <= rec["two_launch"]["median_us"]
            print(json.dumps(rec))
            out.append(rec)
    return out


def _wide_cfg(tmp, nc):
    from build_utils.parse_config import materialize_cfg
    path = materialize_cfg(TARGET)
    if nc == 1:
        return path
    text = open(path).read()
    text, n1 = re.subn(r"classes\s*=\s*1\b", "classes=%d" % nc, text)
    text, n2 = re.subn(r"filters\s*=\s*18\b", "filters=%d" % (3 * (5 + nc)), text)
    assert n1 == 3 and n2 == 3, (n1, n2)
    out = os.path.join(tmp, "%s_nc%d.cfg" % (TARGET, nc))
    with open(out, "w") as f:
        f.write(text)
    return out


def model_points(tmp, steps, warmup, B=16, H=512, W=640):
    from build_utils.utils import compute_loss, non_max_suppression
    from dyk import lib as L
    from dyk.optim import FusedAdam
    from models import YOLO
    with open(os.path.join(PKG, "config", "hyp.scratch.4.json")) as f:
        hyp = json.load(f)
    res = {}
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(B, 3, H, W, generator=g).cuda(), torch.rand(B, 3, H, W, generator=g).cuda()
    for nc in (1, 80):
        torch.manual_seed(0)
        m = YOLO(_wide_cfg(tmp, nc))
        m.dyk_dtype = "bf16"
        m = m.cuda()
        m.nc, m.hyp, m.gr = nc, hyp, 1.0
        tg = torch.tensor([[b, (b * 7) % nc, 0.2 + 0.03 * b, 0.5, 0.08, 0.3] for b in range(B)], dtype=torch.float32).cuda()
        opt = FusedAdam(m, lr=1e-4)
        m.train()

        def step():
            ld = compute_loss(m(x, y), tg, m)
            (ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]).backward()
            opt.step()

        def ms(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = []
            for _ in range(n):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            return ts
        ms(step, warmup)
        tr = ms(step, steps)
        m.eval()
        with torch.no_grad():
            ms(lambda: m(x, y), warmup)
            ev = ms(lambda: m(x, y), steps)
            io, _ = m(x, y)
        rec = {"train_step_ms": {"median": round(statistics.median(tr), 3), "min": round(min(tr), 3), "max": round(max(tr), 3), "n": len(tr)},
               "eval_forward_ms": {"median": round(statistics.median(ev), 3), "min": round(min(ev), 3), "max": round(max(ev), 3), "n": len(ev)},
               "eval_pairs_per_s": round(B / statistics.median(ev) * 1e3, 1), "io_shape": list(io.shape)}
        thr = float(io[..., 4].flatten().sort().values[-2000])             # ~2000 candidates of the batch pass the objectness test
        for multi in (False, True):
            fn = lambda: non_max_suppression(io, conf_thres=thr * 0.01, iou_thres=0.6, multi_label=multi)      # noqa: E731
            ms(fn, 3)
            t = ms(fn, max(5, steps // 2))
            ws = int(L.load().dyk_nms_workspace_bytes(io.shape[1], io.shape[2], 1 if (multi and nc > 1) else 0)) * B
            rec["nms_multi_label_%s" % multi] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                                                 "max_ms": round(max(t), 3), "n": len(t), "workspace_bytes": ws}
        print(json.dumps({"classes": nc, **rec}))
        res["classes_%d" % nc] = rec
        del m, opt
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer samples (a functional check of the probe itself)")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_heads.json"))
    a = ap.parse_args()
    from dyk.buildinfo import native_sha
    rounds, samples, batch = (2, 5, 20) if a.quick else (5, 20, 50)
    res = {"tool": "wide_head_probe", "device": torch.cuda.get_device_name(0), "library": native_sha(),
           "method": "legs interleaved in %d rounds of %d samples; a sample = mean of %d back-to-back launches between two events; "
                     "spread = (max - min) / median over the samples" % (rounds, samples, batch),
           "kernel": kernel_points(rounds, samples, batch)}
    res["fused_not_slower_at_every_point"] = all(r["fused_not_slower"] for r in res["kernel"])
    try:
        with open(os.path.join(ROOT, "profiles", "tensor_stats.json")) as f:
            ts = json.load(f)["kernels"]
        res["bandwidth_bound_kernels_GB_per_s"] = {k: v["GB_per_s"] for k, v in ts.items()}
    except (OSError, KeyError):
        pass
    def write():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", a.out)
    write()
    if not a.no_model:
        with tempfile.TemporaryDirectory() as tmp:
            res["model"] = model_points(tmp, 5 if a.quick else 20, 3 if a.quick else 8)
        write()


if __name__ == "__main__":
    main()
