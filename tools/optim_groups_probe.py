"""What the fused optimizer step launch costs, entry by entry, in ONE process (GPU): the step launch alone on buffers of the target
cfg's flat parameter store (p, g, m, v fp32, the bf16 copy written, g cleared -- the launch FusedAdam / FusedSGD.step() makes),
device events around `iters` back-to-back launches after warm-up, legs alternating over `rounds` rounds.  For Adam and SGD:

  plain        dyk_<rule>_step without a mask
  masked       dyk_<rule>_step with the group map binarised       (what a model with frozen layers pays for the byte)
  guarded      dyk_<rule>_step_guarded with a record of coef = 1, applied = 10
  groups       dyk_<rule>_step_groups with the three groups of dyk.optim.yolo_param_groups
  groups_rec   ... and that record

With --parent-lib (ANOTHER build of the library, e.g. the parent commit's) every leg runs from both libraries on the same buffers,
parent first, and `within` says per leg whether  median(this build) <= median(parent) + the larger of the two spreads over rounds.
Expected for groups against plain: one more byte per element on 4+4+4+4 (p, g, m, v read) + 4+4+4+4 (p, m, v, g written) + 2
(bf16 copy) = 34 bytes, i.e. 35/34 of the traffic (Adam; SGD moves no v: 26 bytes).  Prints one JSON document headed by the code
hash; --out FILE also writes it.
usage: python tools/optim_groups_probe.py [--rounds 5] [--iters 50] [--parent-lib libdyk_hip.so] [--out profiles/optim_unify.json]"""
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
# leg -> (entry suffix, mask: None | "binary" | "groups", group table, record)
LEGS = {"plain": ("", None, False, False), "masked": ("", "binary", False, False), "guarded": ("_guarded", None, False, True),
        "groups": ("_groups", "groups", True, False), "groups_rec": ("_groups", "groups", True, True)}


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
    libs = {"new": L.load()}
    if a.parent_lib:
        par = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for rule in ("adam", "sgd"):
            for suffix in ("", "_guarded", "_groups"):
                name = "dyk_%s_step%s" % (rule, suffix)
                getattr(par, name).restype, getattr(par, name).argtypes = L.SIGNATURES[name]
        libs = {"parent": par, "new": libs["new"]}
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
    masks = {"groups": torch.from_numpy(gmap_host).cuda()}
    masks["binary"] = (masks["groups"] != 0).to(torch.uint8)
    r = L.DykGradGuardRec()
    r.coef, r.applied, r.bc1, r.bc2_sqrt = 1.0, 10, 1.0 - 0.937 ** 10, (1.0 - 0.999 ** 10) ** 0.5
    rec = torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8).cuda()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def leg(lib, rule, suffix, mask, with_table, with_rec):
        d = L.DykOptimDesc()
        d.p, d.g, d.m, d.v, d.wc = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), wc.data_ptr()
        d.mask = masks[mask].data_ptr() if mask else None
        d.n, d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale, d.step, d.zero_grad = n, 1e-3, 0.937, 0.999, 1e-8, 5e-4, 1.0, 10, 1
        fn = getattr(lib, "dyk_%s_step%s" % (rule, suffix))
        rp = ctypes.c_void_p(rec.data_ptr()) if with_rec else None
        if with_table:
            return lambda: fn(ctypes.byref(d), ctypes.byref(table), rp, stream())
        return (lambda: fn(ctypes.byref(d), rp, stream())) if with_rec else (lambda: fn(ctypes.byref(d), stream()))
    legs = [("%s_%s" % (rule, name), which, leg(lib, rule, *spec))
            for rule in ("adam", "sgd") for name, spec in LEGS.items() for which, lib in libs.items()]
    for _, _, fn in legs:
        for _ in range(a.warmup):
            assert fn() == 0
    torch.cuda.synchronize()
    us = {(name, which): [] for name, which, _ in legs}
    for _ in range(a.rounds):
        for name, which, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                assert fn() == 0
            e1.record()
            e1.synchronize()
            us[(name, which)].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    med = {k: float(np.median(t)) for k, t in us.items()}
    spread = {k: float(max(t) - min(t)) for k, t in us.items()}
    doc = {"code_sha": code_sha(), "device": torch.cuda.get_device_name(0), "cfg": TARGET, "elements": n,
           "share_of_elements_by_mask_byte": share,
           "timed": "the step launch alone (bf16 copy written, g cleared), us per launch = device-event time of %d back-to-back "
                    "launches / %d; median of %d rounds, legs alternating" % (a.iters, a.iters, a.rounds),
           "legs": {}}
    for name in dict.fromkeys(name for name, _, _ in legs):
        row = {which: {"us_per_launch": round(med[(name, which)], 2), "spread_over_rounds_us": round(spread[(name, which)], 2),
                       "us_rounds": [round(x, 2) for x in us[(name, which)]]} for which in libs}
        if "parent" in libs:
            row["new_minus_parent_us"] = round(med[(name, "new")] - med[(name, "parent")], 2)
            row["within"] = bool(med[(name, "new")] <= med[(name, "parent")] + max(spread[(name, "parent")], spread[(name, "new")]))
        doc["legs"][name] = row
    if "parent" in libs:
        doc["all_within"] = all(row["within"] for row in doc["legs"].values())
    doc["adam_groups_over_plain"] = round(med[("adam_groups", "new")] / med[("adam_plain", "new")], 4)
    doc["adam_groups_within_traffic_ratio_plus_spread"] = bool(
        med[("adam_groups", "new")] <= med[("adam_plain", "new")] * 35 / 34 + spread[("adam_plain", "new")])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
