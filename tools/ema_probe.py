"""Cost of ModelEMA on the benchmark's workload (target cfg, 16 pairs of 640x512, bf16, FusedAdam -- bench.py's step):

  * `ema.update(model)` alone: one dyk_ema_update launch over the flat parameter and running-statistics buffers, median of
    warm calls timed with HIP events, and the effective rate over the bytes it must move (read P, read and write the shadow);
  * the reference's per-entry torch loop (build_utils/torch_utils.py:108-120 of the reference) on the same two models;
  * the train step with and without `ema.update` after it, in alternating blocks of steps (median step time from events).

    python tools/ema_probe.py [--steps 20] [--calls 30] [--out FILE]

Prints a text report (and writes it to --out) headed by the code hash (tools/code_sha.py)."""
import argparse
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402


def timed(fn, n):
    """per-call durations (ms) of n calls of fn, each between two HIP events on the current stream"""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    evs[0].record()
    for i in range(n):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(n))


def median(xs):
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed train steps per block (two blocks with, two without EMA)")
    ap.add_argument("--calls", type=int, default=30, help="timed ema.update calls")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from build_utils.torch_utils import ModelEMA
    from build_utils.utils import compute_loss
    from code_sha import code_sha
    from dyk.optim import FusedAdam
    from models import YOLO

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("ema_probe: code %s, %s, %s" % (code_sha(), torch.cuda.get_device_name(device), bench.use_recorded_tuning(device)))
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = YOLO(bench.model_cfg(bench.CFG))
    model.nc, model.hyp, model.gr = 1, bench.load_hyp(), 1.0
    model.dyk_dtype = "bf16"
    model = model.to(device).train()
    hyp = model.hyp
    B, H, W = args.batch, 512, 640
    v8, l8, targets = bench.synth_batch(B, H, W, 0, device)
    opt = FusedAdam(model, lr=hyp["lr0"] * 0.001, betas=(hyp["momentum"], 0.999), weight_decay=hyp["weight_decay"])

    def step():
        pred = model(v8, l8)
        ld = compute_loss(pred, targets, model)
        (ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]).backward()
        opt.step()

    for _ in range(5):
        step()
    ema = ModelEMA(model)
    for _ in range(3):
        ema.update(model)
    torch.cuda.synchronize()
    st = model.engine.store
    n_float = sum(1 for v in model.state_dict().values() if v.dtype.is_floating_point)
    nbytes = 3 * 4 * (st.total + st.rtotal)
    say("target cfg %s, batch %d bf16: %d floating state_dict entries, P %d + R %d floats, update moves %.3f GB"
        % (bench.CFG, B, n_float, st.total, st.rtotal, nbytes / 1e9))

    t = timed(lambda: ema.update(model), args.calls)
    say("ema.update (one dyk_ema_update launch): median %.4f ms, min %.4f, max %.4f over %d warm calls -> %.2f TB/s effective"
        % (median(t), t[0], t[-1], len(t), nbytes / (median(t) * 1e-3) / 1e12))

    esd, msd = ema.ema.state_dict(), model.state_dict()

    def reference_loop():
        d = ema.decay(ema.updates)
        with torch.no_grad():
            for k, v in esd.items():
                if v.dtype.is_floating_point:
                    v *= d
                    v += (1. - d) * msd[k].detach()
    for _ in range(2):
        reference_loop()
    t = timed(reference_loop, max(args.calls // 3, 5))
    say("reference per-entry torch loop (%d entries, 3 torch kernels each): median %.3f ms, min %.3f, max %.3f over %d calls"
        % (n_float, median(t), t[0], t[-1], len(t)))
    ema.ema.engine.store.mark_dirty()

    def with_ema():
        step()
        ema.update(model)
    blocks = {"without": [], "with": []}
    for _ in range(2):
        for name, fn in (("without", step), ("with", with_ema)):
            fn()
            blocks[name] += timed(fn, args.steps)
    for name in ("without", "with"):
        t = sorted(blocks[name])
        say("train step %-7s ema.update: median %.3f ms, mean %.3f, min %.3f, max %.3f over %d steps"
            % (name, median(t), sum(t) / len(t), t[0], t[-1], len(t)))
    a, b = sorted(blocks["without"]), sorted(blocks["with"])
    say("train step cost of ema.update: %+.3f ms (median), %+.3f ms (mean)"
        % (median(b) - median(a), sum(b) / len(b) - sum(a) / len(a)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
