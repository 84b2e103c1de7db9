"""Cost of the gradient guard on the benchmark's workload (target cfg, 16 pairs of 640x512, bf16, FusedAdam -- bench.py's step).

One process, one model; the legs alternate in rounds, every leg is warmed and then timed per step with HIP events:

  a1, a2  plain FusedAdam.step()  (the default path; run twice per round: |a1 - a2| is the run-to-run spread)
  b       FusedAdam(skip_nonfinite=True, max_grad_norm=10).step()
  c       the reference harness's way: torch.amp.GradScaler -- scaler.scale(loss).backward(); scaler.step(opt); scaler.update()
  d       torch.nn.utils.clip_grad_norm_(model.parameters(), 10) + plain step
  e       dyk.optim.clip_grad_norm_(model, 10) + plain step

and dyk_grad_stats alone over the model's gradient buffer (both launches between two events; the bytes are the 4 n it must
read), and over a 4 MB buffer that still fills the capped grid (partials negligible: the fold and the two launches).

    python tools/grad_guard_probe.py [--steps 20] [--rounds 2] [--out profiles/grad_guard.json]

Every block of steps runs under a watchdog (--timeout seconds): a hung step ends the process with a traceback instead of
waiting.  Writes one JSON file headed by the code hash (tools/code_sha.py)."""
import argparse
import contextlib
import faulthandler
import json
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
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


def summary(ts):
    s = sorted(ts)
    return dict(median_ms=round(s[len(s) // 2], 4), mean_ms=round(sum(s) / len(s), 4), min_ms=round(s[0], 4),
                max_ms=round(s[-1], 4), n=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed train steps per leg and round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=50, help="timed dyk_grad_stats calls")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=120, help="watchdog per block of steps, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard.json"))
    args = ap.parse_args()
    import bench
    from build_utils.utils import compute_loss
    from code_sha import code_sha
    from dyk import ops
    from dyk.optim import FusedAdam, clip_grad_norm_
    from models import YOLO

    assert torch.cuda.is_available(), "grad_guard_probe measures on the GPU only"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = dict(tool="grad_guard_probe", code=code_sha(), device=torch.cuda.get_device_name(device),
               tuning=str(bench.use_recorded_tuning(device)), cfg=bench.CFG, batch=args.batch, dtype="bf16",
               steps_per_leg_and_round=args.steps, rounds=args.rounds)
    print(json.dumps(res), flush=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = YOLO(bench.model_cfg(bench.CFG))
    model.nc, model.hyp, model.gr = 1, bench.load_hyp(), 1.0
    model.dyk_dtype = "bf16"
    model = model.to(device).train()
    hyp = model.hyp
    B, H, W = args.batch, 512, 640
    v8, l8, targets = bench.synth_batch(B, H, W, 0, device)
    kw = dict(lr=hyp["lr0"] * 0.001, betas=(hyp["momentum"], 0.999), weight_decay=hyp["weight_decay"])
    plain = FusedAdam(model, **kw)
    guarded = FusedAdam(model, skip_nonfinite=True, max_grad_norm=10.0, **kw)
    scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=10 ** 9)   # bf16: a non-finite guard only
    params = [p for p in model.parameters()]

    def loss():
        ld = compute_loss(model(v8, l8), targets, model)
        return ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]

    def leg_a():
        loss().backward()
        plain.step()

    def leg_b():
        loss().backward()
        guarded.step()

    def leg_c():
        scaler.scale(loss()).backward()
        scaler.step(plain)
        scaler.update()

    def leg_d():
        loss().backward()
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        plain.step()

    def leg_e():
        loss().backward()
        clip_grad_norm_(model, 10.0)
        plain.step()

    legs = [("a1", leg_a), ("b", leg_b), ("c", leg_c), ("d", leg_d), ("e", leg_e), ("a2", leg_a)]
    times = {name: [] for name, _ in legs}
    faulthandler.dump_traceback_later(args.timeout * 3, exit=True)
    for _ in range(5):
        leg_a()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, fn in legs:
            faulthandler.dump_traceback_later(args.timeout, exit=True)
            fn()
            fn()
            times[name] += timed(fn, args.steps)
            print("round %d leg %-2s median %.3f ms" % (r, name, summary(times[name][-args.steps:])["median_ms"]), flush=True)
    faulthandler.cancel_dump_traceback_later()
    res["train_step"] = {name: summary(t) for name, t in times.items()}
    med = {k: v["median_ms"] for k, v in res["train_step"].items()}
    res["spread_a_ms"] = round(abs(med["a1"] - med["a2"]), 4)
    res["a_ms"] = round((med["a1"] + med["a2"]) / 2, 4)
    res["b_minus_a_ms"] = round(med["b"] - res["a_ms"], 4)
    res["b_minus_c_ms"] = round(med["b"] - med["c"], 4)
    res["e_minus_d_ms"] = round(med["e"] - med["d"], 4)
    res["b_not_slower_than_c"] = bool(med["b"] <= med["c"] + res["spread_a_ms"])
    res["e_not_slower_than_d"] = bool(med["e"] <= med["d"] + res["spread_a_ms"])
    res["guarded_stats"] = guarded.grad_stats(wait=True)

    st = model.engine.store
    faulthandler.dump_traceback_later(args.timeout, exit=True)
    rec, ws = ops.grad_guard_record(device), ops.grad_stats_workspace(st.total, device)

    def stats_full():
        ops.grad_stats(st.G, rec, ws, max_norm=10.0, skip_nonfinite=True)
    small = torch.zeros(1024 * 256 * 4, device=device)
    ws_small = ops.grad_stats_workspace(small.numel(), device)

    def stats_small():
        ops.grad_stats(small, rec, ws_small, max_norm=10.0, skip_nonfinite=True)
    for name, fn, nbytes in (("full", stats_full, 4 * st.total), ("small", stats_small, 4 * small.numel())):
        for _ in range(5):
            fn()
        s = summary(timed(fn, args.calls))
        s["bytes"] = nbytes
        s["GB_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 1)
        res["grad_stats_" + name] = s
    faulthandler.cancel_dump_traceback_later()
    res["ema_kernel_TB_per_s"] = 4.89            # profiles/r07_ema_probe.txt
    res["stats_vs_ema_bandwidth"] = round(res["grad_stats_full"]["GB_per_s"] / 4890.0, 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
