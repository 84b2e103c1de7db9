"""What merge-NMS (DYK_NMS_MERGE, reference build_utils/utils.py:450-454) costs and what it buys, in ONE process (GPU).
The NMS launch alone (dyk_nms / dyk_nms_ex on preallocated buffers, device events around `iters` back-to-back launches, after
warm-up) on three inputs of 16 images built from tests/golden/cases.py and tests/nms_merge_ref.py:
  dense   16 x the `dense` case  (20 160 candidates per image: the no-merge branch of :450),
  sparse  16 x the `sparse` case (about 300 candidates per image),
  worst   16 images with n = 2999 candidates and 100 kept boxes (the most merge work one image can have).
Legs alternate and every leg runs twice per round (plain, merge, plain_again, merge_again), so the spread between equal legs is
known.  `--parent-lib FILE` adds two legs that call dyk_nms of another build of the library (the parent commit's) on the same
buffers in the same process: the plain leg runs the same kernel code, so it has to agree with them within that spread.
Then the fp32 eval chain of the 64-pair fixture (tests/golden/evalap_trained64.npz) once without and once with merge:
AP / LAMR / detections beside the CPU values of the restatement on the recorded `io`.  Prints one JSON document with the
code hash; `--out FILE` also writes it.
usage: python tools/nms_merge_probe.py [--rounds 7] [--iters 20] [--parent-lib libdyk_hip.so] [--out profiles/nms_merge.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CPU_VALUES = {"plain": {"ap": 0.7544514607, "lamr": 0.4836055601, "detections": 910},
              "merged": {"ap": 0.7560124325, "lamr": 0.4836055601, "detections": 910}}


class Launch:
    """one NMS problem with its buffers and descriptor; run(fn, flags) issues one launch"""

    def __init__(self, L, pred, conf, iou):
        self.pred = pred.cuda().contiguous()
        B, N, no = self.pred.shape
        h = L.load()
        per = int(h.dyk_nms_workspace_bytes(N, no, 0))
        self.ws = torch.empty(B * per, dtype=torch.uint8, device="cuda")
        self.out = torch.zeros((B, 100, 6), device="cuda")
        self.rows = torch.zeros((B, 100), dtype=torch.int32, device="cuda")
        self.counts = torch.zeros(B, dtype=torch.int32, device="cuda")
        d = self.d = L.DykNmsDesc()
        d.pred, d.out, d.out_rows, d.counts, d.ws, d.ws_per_image = (self.pred.data_ptr(), self.out.data_ptr(), self.rows.data_ptr(),
                                                                     self.counts.data_ptr(), self.ws.data_ptr(), per)
        d.B, d.N, d.no, d.conf_thres, d.iou_thres = B, N, no, conf, iou
        d.multi_label, d.agnostic, d.max_num, d.n_classes = 0, 0, 100, 0

    def run(self, fn, flags):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = fn(ctypes.byref(self.d), s) if flags is None else fn(ctypes.byref(self.d), flags, s)
        assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cases
    import nms_merge_ref as ref
    from code_sha import code_sha
    from dyk import lib as L
    h = L.load()
    legs = [("plain", h.dyk_nms_ex, 0), ("merge", h.dyk_nms_ex, L.NMS_MERGE), ("plain_again", h.dyk_nms_ex, 0),
            ("merge_again", h.dyk_nms_ex, L.NMS_MERGE)]
    if a.parent_lib:
        par = ctypes.CDLL(os.path.abspath(a.parent_lib))
        par.dyk_nms.restype, par.dyk_nms.argtypes = ctypes.c_int32, [ctypes.POINTER(L.DykNmsDesc), ctypes.c_void_p]
        legs += [("parent_dyk_nms", par.dyk_nms, None), ("parent_dyk_nms_again", par.dyk_nms, None)]
    by_name = {c["name"]: c for c in cases.nms_cases()}
    inputs = {}
    for name in ("dense", "sparse"):
        c = dict(by_name[name], B=16)
        inputs[name] = (cases.nms_pred(c), c["conf"], c["iou"])
    inputs["worst"] = (ref.cluster_rows(16, 2999, 9, ncl=120), 0.25, 0.6)
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0),
           "timed": "the NMS launch alone, 16 images, us per launch = device-event time of %d back-to-back launches / %d; median of "
                    "%d rounds, legs alternating" % (a.iters, a.iters, a.rounds), "inputs": {}}
    for name, (pred, conf, iou) in inputs.items():
        p = Launch(L, pred, conf, iou)
        info = {}
        if name != "dense":                     # (the CPU restatement of 16 x 20 160 candidates takes minutes and says n = 20 160)
            ref.non_max_suppression(pred[:2], conf, iou, False, merge=False, info=info)
        for _, fn, flags in legs:
            for _ in range(a.warmup):
                p.run(fn, flags)
        torch.cuda.synchronize()
        us = {leg: [] for leg, _, _ in legs}
        for _ in range(a.rounds):
            for leg, fn, flags in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    p.run(fn, flags)
                e1.record()
                e1.synchronize()
                us[leg].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med = {leg: float(np.median(v)) for leg, v in us.items()}
        p.run(h.dyk_nms_ex, L.NMS_MERGE)
        rec = {"candidates_per_image": "20160" if name == "dense" else "%d..%d (first two images)" % (min(info["n"]), max(info["n"])),
               "kept_per_image": sorted(set(p.counts.cpu().tolist())),
               "us_per_launch": {leg: round(med[leg], 2) for leg in med},
               "us_rounds": {leg: [round(t, 2) for t in v] for leg, v in us.items()},
               "merge_cost_us": round((med["merge"] + med["merge_again"] - med["plain"] - med["plain_again"]) / 2, 2),
               "spread_of_equal_legs_us": {"plain": round(abs(med["plain"] - med["plain_again"]), 2),
                                           "merge": round(abs(med["merge"] - med["merge_again"]), 2)}}
        if a.parent_lib:
            rec["plain_minus_parent_us"] = round((med["plain"] + med["plain_again"] - med["parent_dyk_nms"] - med["parent_dyk_nms_again"]) / 2, 2)
            rec["spread_of_equal_legs_us"]["parent"] = round(abs(med["parent_dyk_nms"] - med["parent_dyk_nms_again"]), 2)
        doc["inputs"][name] = rec
    # what it buys: the fp32 eval chain of the 64-pair fixture without and with merge
    import make_golden_round4 as R4
    import make_golden_round5 as R5
    from build_utils.parse_config import materialize_cfg
    from build_utils.utils import non_max_suppression, scale_coords
    from helpers import GOLDEN, oracle_net
    from models import YOLO
    from other_utils.metrics import compute_ap_lamr
    gold = np.load(os.path.join(GOLDEN, "evalap_trained64.npz"))
    net = oracle_net(R5.CFG)
    sd = R4.conditioned_state(net.synth_state(R5.SEED_W))
    for k in gold.files:
        if k.startswith(("bn|", "head|")):
            sd[k.split("|", 1)[1]] = torch.from_numpy(gold[k])
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(R5.CFG))
    m.load_state_dict(sd)
    m.dyk_dtype = "fp32"
    m = m.cuda().eval()
    v, l, targets = R5.dataset()
    labels, shapes = R5.labels_of(targets)
    with torch.no_grad():
        io = torch.cat([m(v[c:c + 16].cuda().float() / 255.0, l[c:c + 16].cuda().float() / 255.0)[0].clone() for c in range(0, 64, 16)])
    doc["fixture"] = {"file": "tests/golden/evalap_trained64.npz", "chain": "fp32 forward + decode + NMS + scale_coords + AP evaluator",
                      "cpu_restatement_on_the_recorded_io": CPU_VALUES}
    for name, merge in (("plain", False), ("merged", True)):
        dets = non_max_suppression(io, conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False, merge=merge)
        preds = []
        for idx, p in enumerate(dets):
            if p is None:
                continue
            boxes = scale_coords((R5.H, R5.W), p[:, :4].clone(), R5.SHAPE0, R5.RATIO_PAD).cpu().numpy()
            conf = p[:, 4].cpu().numpy()
            preds += [{"img_id": idx, "conf": float(conf[i]), "bbox": boxes[i]} for i in range(boxes.shape[0])]
        preds.sort(key=lambda q: q["conf"], reverse=True)
        res = compute_ap_lamr(preds, [lb.copy() for lb in labels], shapes)
        doc["fixture"][name] = {"ap": round(float(res["ap"]), 10), "lamr": round(float(res["lamr"]), 10), "detections": len(preds)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
