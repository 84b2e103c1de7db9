"""Evaluation throughput and accuracy of the three arithmetic modes (fp32, bf16, fp16) in ONE process (GPU).
Target cfg, batch 16, 640x512: forward + decode + NMS timed for fp32 / bf16 / bf16 again / fp16, alternating after warm-up (the
second bf16 leg measures the run-to-run spread the fp16 / bf16 ratio has to be read against); then AP / LAMR / detections of
each mode on the 64-pair fixture (tests/golden/evalap_trained64.npz); then every launch of the bf16 and of the fp16 forward
plan timed alone on the chip (dyk_run_schedule_timed, best of three), summed per kernel family, with the commands whose fp16
time exceeds their bf16 time most -- where a missed fp16 / bf16 ratio comes from.  Prints one JSON document (with the code hash, as the other
profiles carry it); `--out FILE` also writes it.
usage: python tools/eval_precision.py [--rounds 5] [--iters 10] [--out profiles/fp16_eval.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "tools")]
import ctypes  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _family(L, op, d):
    """kernel family of one command: the op's name; convolutions by the tile family their tune word selects"""
    name = {v: k[3:].lower() for k, v in vars(L).items() if k.startswith("OP_") and isinstance(v, int)}.get(op, "op%d" % op)
    if op != L.OP_CONV:
        return name
    tile = (d.tune >> 12) & 0xf
    fam = {5: "large-tile", 7: "pointwise", 3: "halo", 4: "halo"}.get(tile, "generic")
    if (d.tune >> 28) & 7 == 1:
        fam = "k-grouped"
    return "conv " + fam + (" split-K" if d.splitk > 1 else "")


def isolated_times(plan, reps=3):
    """us of every forward command of the plan, each launch alone on the chip (best of `reps`) -> {cmd index: us}"""
    from dyk import lib as L
    sc = plan.schedule("fwd", 0, len(plan.fwd))
    best = None
    for _ in range(reps):
        ms = (ctypes.c_float * max(sc.n, 1))()
        L.check(L.load().dyk_run_schedule_timed(plan._cfwd, sc.array, sc.n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ms),
                "dyk_run_schedule_timed")
        t = [float(v) * 1e3 for v in ms]
        best = t if best is None else [min(a, b) for a, b in zip(best, t)]
    out = {}
    for e, t in zip(sc.entries, best):
        out[e["cmd"]] = out.get(e["cmd"], 0.0) + t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import make_golden_round4 as R4
    import make_golden_round5 as R5
    from build_utils.parse_config import materialize_cfg
    from build_utils.utils import non_max_suppression, scale_coords
    from code_sha import code_sha
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
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(0)
    B, H, W = 16, 512, 640
    xv = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    xl = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()

    def step(dt):
        m.dyk_dtype = dt
        with torch.no_grad():
            io, _ = m(xv, xl)
            non_max_suppression(io, conf_thres=0.3, iou_thres=0.6, multi_label=False)

    legs = [("fp32", "fp32"), ("bf16", "bf16"), ("bf16_again", "bf16"), ("fp16", "fp16")]
    for _, dt in legs:
        for _ in range(a.warmup):
            step(dt)
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, dt in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                step(dt)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "cfg": R5.CFG, "batch": B, "size": [W, H],
           "timed": "forward + decode + NMS, %d rounds x %d iterations per leg, legs alternating" % (a.rounds, a.iters),
           "fixture": "tests/golden/evalap_trained64.npz", "modes": {}}
    for name, _ in legs:
        med = float(np.median(ms[name]))
        doc["modes"][name] = {"ms_per_batch": round(med, 4), "pairs_per_s": round(B / med * 1e3, 1),
                              "ms_rounds": [round(t, 4) for t in ms[name]]}
    pb = doc["modes"]["bf16"]["pairs_per_s"]
    doc["fp16_over_bf16"] = round(doc["modes"]["fp16"]["pairs_per_s"] / pb, 4)
    doc["bf16_again_over_bf16"] = round(doc["modes"]["bf16_again"]["pairs_per_s"] / pb, 4)
    # accuracy on the 64-pair fixture
    v, l, targets = R5.dataset()
    labels, shapes = R5.labels_of(targets)
    for dt in ("fp32", "bf16", "fp16"):
        m.dyk_dtype = dt
        with torch.no_grad():
            io = torch.cat([m(v[c:c + 16].cuda().float() / 255.0, l[c:c + 16].cuda().float() / 255.0)[0].clone() for c in range(0, 64, 16)])
        dets = non_max_suppression(io, conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
        preds = []
        for idx, p in enumerate(dets):
            if p is None:
                continue
            boxes = scale_coords((R5.H, R5.W), p[:, :4].clone(), R5.SHAPE0, R5.RATIO_PAD).cpu().numpy()
            conf = p[:, 4].cpu().numpy()
            preds += [{"img_id": idx, "conf": float(conf[i]), "bbox": boxes[i]} for i in range(boxes.shape[0])]
        preds.sort(key=lambda q: q["conf"], reverse=True)
        res = compute_ap_lamr(preds, [lb.copy() for lb in labels], shapes)
        gio = torch.from_numpy(gold["io"])
        doc["modes"][dt].update(ap=round(float(res["ap"]), 5), lamr=round(float(res["lamr"]), 5), detections=len(preds),
                                io_rel_err=float((io.cpu() - gio).abs().max() / gio.abs().max()))
    # where the time goes: isolated time of every forward command of the two 16-bit plans, per kernel family
    from dyk import lib as L
    pb_, ph_ = (m.engine.plans[(B, H, W, dt, False)] for dt in (torch.bfloat16, torch.float16))
    step("bf16")                                   # (points the plan at this batch again)
    tb = isolated_times(pb_)
    step("fp16")
    th = isolated_times(ph_)
    fam = {}
    for name, plan, tt in (("bf16", pb_, tb), ("fp16", ph_, th)):
        for ci, us in tt.items():
            op, d = plan.fwd[ci]
            f = fam.setdefault(_family(L, op, d), {"bf16_us": 0.0, "fp16_us": 0.0, "bf16_n": 0, "fp16_n": 0})
            f[name + "_us"] += us
            f[name + "_n"] += 1
    doc["isolated_forward_us"] = {"bf16": round(sum(tb.values()), 1), "fp16": round(sum(th.values()), 1),
                                  "families": {k: {a: (round(b, 1) if isinstance(b, float) else b) for a, b in v.items()}
                                               for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["fp16_us"])}}
    if len(pb_.fwd) == len(ph_.fwd):
        rows = []
        for ci in th:
            op, d = ph_.fwd[ci]
            if ci in tb:
                row = {"cmd": ci, "family_fp16": _family(L, op, d), "family_bf16": _family(L, *pb_.fwd[ci]), "bf16_us": round(tb[ci], 2),
                       "fp16_us": round(th[ci], 2)}
                if op == L.OP_CONV:
                    row.update(Cin=d.Cin, Cout=d.Cout, Hg=d.Hg, Wg=d.Wg, taps=d.ntaps, tune_fp16=hex(d.tune), tune_bf16=hex(pb_.fwd[ci][1].tune))
                rows.append(row)
        rows.sort(key=lambda r: r["bf16_us"] - r["fp16_us"])
        doc["largest_fp16_excess"] = rows[:8]
    doc["reference"] = {"ap": round(float(gold["ap"]), 5), "lamr": round(float(gold["lamr"]), 5), "detections": int(gold["ndet"].sum())}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
