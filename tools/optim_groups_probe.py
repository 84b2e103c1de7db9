"""What parameter groups cost in the fused Adam step, in ONE process (GPU): the step launch alone on buffers of the target cfg's
flat parameter store (p, g, m, v fp32, the bf16 copy written, g cleared -- the launch FusedAdam.step() makes), device events
around `iters` back-to-back launches after warm-up, legs alternating over `rounds` rounds:

  a         dyk_adam_step without a mask, from ANOTHER build of the library (--parent-lib: the parent commit's), same buffers
  b         this build's dyk_adam_step without a mask              (the same statements: must agree with a within a's spread)
  b_masked  this build's dyk_adam_step with the group map binarised (what a model with frozen layers already pays for the byte)
  c         dyk_adam_step_groups with the three groups of dyk.optim.yolo_param_groups

Expected for c against a: one more byte per element on 4+4+4+4 (p, g, m, v read) + 4+4+4+4 (p, m, v, g written) + 2 (bf16 copy)
= 34 bytes, i.e. 35/34 of the traffic.  Prints one JSON document headed by the code hash; --out FILE also writes it.
usage: python tools/optim_groups_probe.py [--rounds 5] [--iters 50] [--parent-lib libdyk_hip.so] [--out profiles/optim_groups.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

TARGET = "kaist_dyolov4_fshare_global_concat_se3"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from build_utils.parse_config import materialize_cfg
    from code_sha import code_sha
    from dyk import lib as L
    from dyk.optim import FusedAdam, group_map, yolo_param_groups
    from models import YOLO
    h = L.load()
    torch.manual_seed(0)
    model = YOLO(materialize_cfg(TARGET))
    st = model.engine.store
    n = st.total
    opt = FusedAdam(model, lr=1e-3, betas=(0.937, 0.999), param_groups=yolo_param_groups(model, 5e-4, bias_lr=2e-3))
    gmap_host = group_map(st.entries, opt.param_groups, n)
    table = opt._group_table()
    share = {str(k): round(float(np.mean(gmap_host == k)), 5) for k in range(4)}
    gen = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=gen) * 0.1
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    wc = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    gmap = torch.from_numpy(gmap_host).cuda()
    binary = (gmap != 0).to(torch.uint8)

    def desc(mask):
        d = L.DykOptimDesc()
        d.p, d.g, d.m, d.v, d.wc = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), wc.data_ptr()
        d.mask = mask.data_ptr() if mask is not None else None
        d.n, d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale, d.step, d.zero_grad = n, 1e-3, 0.937, 0.999, 1e-8, 5e-4, 1.0, 10, 1
        return d
    plain, masked, grouped = desc(None), desc(binary), desc(gmap)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    legs = [("b", lambda: h.dyk_adam_step(ctypes.byref(plain), stream())),
            ("b_masked", lambda: h.dyk_adam_step(ctypes.byref(masked), stream())),
            ("c", lambda: h.dyk_adam_step_groups(ctypes.byref(grouped), ctypes.byref(table), None, stream()))]
    if a.parent_lib:
        par = ctypes.CDLL(os.path.abspath(a.parent_lib))
        par.dyk_adam_step.restype, par.dyk_adam_step.argtypes = ctypes.c_int32, [ctypes.POINTER(L.DykOptimDesc), ctypes.c_void_p]
        legs.insert(0, ("a", lambda: par.dyk_adam_step(ctypes.byref(plain), stream())))
    for _, fn in legs:
        for _ in range(a.warmup):
            assert fn() == 0
    torch.cuda.synchronize()
    us = {leg: [] for leg, _ in legs}
    for _ in range(a.rounds):
        for leg, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                assert fn() == 0
            e1.record()
            e1.synchronize()
            us[leg].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    med = {leg: float(np.median(t)) for leg, t in us.items()}
    spread = {leg: float(max(t) - min(t)) for leg, t in us.items()}
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "cfg": TARGET, "elements": n,
           "share_of_elements_by_mask_byte": share,
           "timed": "the step launch alone (bf16 copy written, g cleared), us per launch = device-event time of %d back-to-back "
                    "launches / %d; median of %d rounds, legs alternating" % (a.iters, a.iters, a.rounds),
           "us_per_launch": {k: round(x, 2) for k, x in med.items()},
           "spread_over_rounds_us": {k: round(x, 2) for k, x in spread.items()},
           "us_rounds": {k: [round(x, 2) for x in t] for k, t in us.items()},
           "gbytes_per_s": {k: round((35 if k in ("c", "b_masked") else 34) * n / x / 1e3, 1) for k, x in med.items()},
           "traffic_ratio_c_over_a": round(35 / 34, 4)}
    base = "a" if "a" in med else "b"
    doc["c_over_%s" % base] = round(med["c"] / med[base], 4)
    doc["c_within_traffic_ratio_plus_spread"] = bool(med["c"] <= med[base] * 35 / 34 + spread[base])
    if "a" in med:
        doc["b_minus_a_us"] = round(med["b"] - med["a"], 2)
        doc["b_within_spread_of_a"] = bool(abs(med["b"] - med["a"]) <= max(spread["a"], spread["b"]))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
