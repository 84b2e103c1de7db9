"""Does a network fit fp16?  (GPU)  Run this once on your weights before trusting `model.dyk_dtype = "fp16"`.
For a cfg, a checkpoint (or seeded synthetic weights) and a batch, runs the fp32 plan with every section's output kept
(DYK_DEBUG_PLAN=1) and prints the sections' largest |activation| against fp16's 65504; then runs the fp16 plan on the same
batch and counts the elements it SATURATED (stored as +-65504).  fp16 stores saturate instead of producing inf, so an
overflowing net does not go NaN -- it silently clips: any count above zero means "use bf16 or fp32 for these weights".
usage: python tools/fp16_range.py <cfg-name> [--weights ckpt.pt | --seed N] [--batch 2] [--size 128x160] [--top 10]"""
import argparse
import os
import sys
os.environ["DYK_DEBUG_PLAN"] = "1"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

F16_MAX = 65504.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cfg")
    ap.add_argument("--weights", default=None, help="checkpoint: a state_dict, or a dict with it under 'model'")
    ap.add_argument("--seed", type=int, default=0, help="seed of the synthetic weights and of the batch")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", default="128x160", help="HxW, multiples of 32")
    ap.add_argument("--top", type=int, default=10)
    a = ap.parse_args()
    from build_utils.parse_config import materialize_cfg
    from gpu_debug_model import tref_to_nchw
    from models import YOLO
    H, W = (int(s) for s in a.size.lower().split("x"))
    torch.manual_seed(a.seed)
    m = YOLO(materialize_cfg(a.cfg))
    if a.weights:
        ck = torch.load(a.weights, map_location="cpu")
        m.load_state_dict(ck["model"] if isinstance(ck, dict) and "model" in ck else ck)
    else:
        from helpers import oracle_net
        m.load_state_dict(oracle_net(a.cfg).synth_state(a.seed))
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(a.seed)
    x, y = torch.rand(a.batch, 3, H, W, generator=g).cuda(), torch.rand(a.batch, 3, H, W, generator=g).cuda()

    def run(dt):
        m.dyk_dtype = dt
        with torch.no_grad():
            io, _ = m(x, y)
        torch.cuda.synchronize()
        plan = [p for k, p in m.engine.plans.items() if str(k[3]).endswith({"fp32": "float32", "fp16": "float16"}[dt])][0]
        return io, plan
    _, p32 = run("fp32")
    rows = []
    for i, t in enumerate(p32.outs):
        if t is not None and p32.info[i]["kind"] != "yolo":
            rows.append((float(tref_to_nchw(p32, t).abs().max()), i, p32.info[i]["kind"]))
    rows.sort(reverse=True)
    print("%s, batch %d at %dx%d: largest |activation| per section in fp32 (fp16 max %.0f)" % (a.cfg, a.batch, H, W, F16_MAX))
    for v, i, kind in rows[:a.top]:
        print("  section %4d %-24s %12.4g  = %8.4f of the fp16 range%s" % (i, kind, v, v / F16_MAX, "   OVERFLOWS" if v > F16_MAX else ""))
    io16, p16 = run("fp16")
    sat = total = 0
    where = []
    for i, t in enumerate(p16.outs):
        if t is not None and p16.info[i]["kind"] != "yolo" and t.esize == 2:
            v = tref_to_nchw(p16, t)
            n = int((v.abs() >= F16_MAX).sum())
            sat, total = sat + n, total + v.numel()
            if n:
                where.append((n, i, p16.info[i]["kind"]))
    print("fp16 run: %d of %d stored elements saturated at +-%.0f; output finite: %s" % (sat, total, F16_MAX, bool(torch.isfinite(io16).all())))
    for n, i, kind in sorted(where, reverse=True)[:a.top]:
        print("  section %4d %-24s %d saturated" % (i, kind, n))
    fits = sat == 0 and rows[0][0] <= F16_MAX
    print("verdict: %s" % ("fits fp16 on this batch" if fits else "does NOT fit fp16: use bf16 or fp32"))
    return 0 if fits else 2


if __name__ == "__main__":
    sys.exit(main())
