"""Cost of the per-tensor statistics (dyk_tensor_stats, dyk.monitor.TensorStats) on the target cfg's parameter store.

One process; the legs alternate in rounds, every leg is warmed and then timed per call with HIP events:

  (a) the two dyk_tensor_stats launches over G alone (nbuf = 1) against the two dyk_grad_stats launches over the same buffer --
      the yardstick reads the same bytes once through a capped grid.  --parent-lib names the library dyk_grad_stats is taken
      from (a build of the parent commit); without it the in-tree library's is used (csrc/optim_guard.hip is the same file).
  (b) the same for nbuf = 2 (P + G) and nbuf = 4 (P + G + two moment-sized buffers), as time per byte read
  (c) the train step (batch 16, bf16, FusedAdam -- bench.py's step), two legs each:
        a1, a2  plain step
        t       TensorStats(what=("grad",)).launch() between backward() and step(), every step
        p       the torch way: a loop of p.grad.norm() and torch.isfinite(p.grad).all() over the parameters, stacked and read
                with one synchronisation per step

    python tools/tensor_stats_probe.py [--calls 50] [--steps 20] [--rounds 2] [--skip-step] [--out profiles/tensor_stats.json]

(a) and (b) are written to the output before (c) starts.  Every block runs under a watchdog (--timeout seconds)."""
import argparse
import contextlib
import ctypes
import faulthandler
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from grad_guard_probe import summary, timed  # noqa: E402


def write(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="timed calls per kernel leg and round")
    ap.add_argument("--steps", type=int, default=20, help="timed train steps per leg and round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=120, help="watchdog per block, seconds")
    ap.add_argument("--parent-lib", default=None, help="library whose dyk_grad_stats is the yardstick of (a)")
    ap.add_argument("--skip-step", action="store_true", help="(a) and (b) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_stats.json"))
    args = ap.parse_args()
    import bench
    from build_utils.utils import compute_loss
    from code_sha import code_sha
    from dyk import lib as L
    from dyk import ops
    from dyk.buildinfo import native_sha
    from dyk.monitor import TensorStats
    from dyk.optim import FusedAdam
    from models import YOLO

    assert torch.cuda.is_available(), "tensor_stats_probe measures on the GPU only"
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = dict(tool="tensor_stats_probe", code=code_sha(), library=L.load().dyk_build_sha().decode(), tree=native_sha(),
               device=torch.cuda.get_device_name(device), cfg=bench.CFG, batch=args.batch, dtype="bf16",
               calls_per_leg_and_round=args.calls, steps_per_leg_and_round=args.steps, rounds=args.rounds)
    if not args.skip_step:
        res["tuning"] = str(bench.use_recorded_tuning(device))
    print(json.dumps(res), flush=True)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = YOLO(bench.model_cfg(bench.CFG))
    model.nc, model.hyp, model.gr = 1, bench.load_hyp(), 1.0
    model.dyk_dtype = "bf16"
    model = model.to(device).train()
    st = model.engine.store
    if st.P is None:
        with torch.no_grad():
            st.adopt(device)

    # ------------------------------------------------------------------ (a), (b): the launches alone
    faulthandler.dump_traceback_later(args.timeout, exit=True)
    params, _ = st.segment_table()
    table = ops.tensor_stats_worklist([(o, n, 0) for _, o, n in params], device)
    res["elements"], res["segments"], res["items"] = st.total, table["nseg"], table["nitems"]
    res["live_elements"] = sum(n for _, _, n in params)
    live = torch.zeros(st.total, device=device)
    for _, o, n in params:
        live[o:o + n] = 1.0
    g = torch.randn(st.total, device=device) * 1e-2 * live          # (padding zero as in the store: both reductions sum the same values)
    del live
    m1, m2 = torch.randn(st.total, device=device) * 1e-3, torch.rand(st.total, device=device) * 1e-6
    sets = {1: [g], 2: [st.P, g], 4: [st.P, g, m1, m2]}
    out = {k: torch.zeros(table["nseg"] * k * ops.TSTAT_BYTES, dtype=torch.uint8, device=device) for k in sets}
    ws = {k: ops.tensor_stats_workspace(table["nitems"], k, device) for k in sets}
    rec, gws = ops.grad_guard_record(device), ops.grad_stats_workspace(st.total, device)
    if args.parent_lib:
        base = ctypes.CDLL(os.path.abspath(args.parent_lib))
        base.dyk_grad_stats.restype = ctypes.c_int32
        base.dyk_grad_stats.argtypes = [ctypes.POINTER(L.DykGradStatsDesc), ctypes.c_void_p]
        base.dyk_build_sha.restype = ctypes.c_char_p
        res["grad_stats_library"] = "%s (source digest %s)" % (os.path.basename(args.parent_lib), base.dyk_build_sha().decode())
        d = L.DykGradStatsDesc()
        d.g, d.ws, d.rec, d.n, d.ws_bytes = g.data_ptr(), gws.data_ptr(), rec.data_ptr(), st.total, gws.numel()
        d.grad_scale, d.max_norm, d.skip_nonfinite = 1.0, 10.0, 1

        def grad_stats():
            L.check(base.dyk_grad_stats(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dyk_grad_stats")
    else:
        res["grad_stats_library"] = "in-tree"

        def grad_stats():
            ops.grad_stats(g, rec, gws, max_norm=10.0, skip_nonfinite=True)
    legs = [("grad_stats", grad_stats, 1)] + [("tensor_stats_%d" % k, (lambda k=k: ops.tensor_stats(sets[k], table, out[k], ws[k], n=st.total)), k)
                                              for k in sets]
    times = {name: [] for name, _, _ in legs}
    for r in range(args.rounds):
        for name, fn, _ in legs:
            for _ in range(5):
                fn()
            times[name] += timed(fn, args.calls)
    res["kernels"] = {}
    for name, _, k in legs:
        s = summary(times[name])
        s["bytes"] = 4 * st.total * k if name == "grad_stats" else 4 * res["live_elements"] * k
        s["GB_per_s"] = round(s["bytes"] / (s["median_ms"] * 1e-3) / 1e9, 1)
        s["ps_per_byte"] = round(s["median_ms"] * 1e9 / s["bytes"], 4)
        res["kernels"][name] = s
        print(name, json.dumps(s), flush=True)
    res["tensor_stats_1_over_grad_stats"] = round(res["kernels"]["tensor_stats_1"]["median_ms"] / res["kernels"]["grad_stats"]["median_ms"], 3)
    res["target_1_25_met"] = bool(res["tensor_stats_1_over_grad_stats"] <= 1.25)
    # the records of the three buffer counts agree bit for bit on the buffers they share, and the total agrees with the guard
    r1 = ops.tensor_stats_records(out[1].cpu().numpy().tobytes(), table["nseg"], 1)
    r4 = ops.tensor_stats_records(out[4].cpu().numpy().tobytes(), table["nseg"], 4)
    res["nbuf_1_equals_nbuf_4"] = bool(r1[:, 0].tobytes() == r4[:, 1].tobytes())
    import math
    res["norm_from_records"] = math.sqrt(math.fsum(float(x) for x in r1[:, 0]["sumsq"]))
    res["norm_from_grad_stats"] = float(ops.read_grad_record(rec).norm)
    faulthandler.cancel_dump_traceback_later()
    write(res, args.out)
    if args.skip_step:
        print(json.dumps(res, sort_keys=True), flush=True)
        return
    del g, m1, m2, sets, out, ws

    # ------------------------------------------------------------------ (c): the train step
    hyp = model.hyp
    B, H, W = args.batch, 512, 640
    v8, l8, targets = bench.synth_batch(B, H, W, 0, device)
    opt = FusedAdam(model, lr=hyp["lr0"] * 0.001, betas=(hyp["momentum"], 0.999), weight_decay=hyp["weight_decay"])
    stats = TensorStats(model, what=("grad",))
    plist = [p for p in model.parameters()]
    seen = []

    def loss():
        ld = compute_loss(model(v8, l8), targets, model)
        return ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]

    def leg_a():
        loss().backward()
        opt.step()

    def leg_t():
        loss().backward()
        stats.launch()
        opt.step()
        stats.read()

    def leg_p():
        loss().backward()
        norms = torch.stack([p.grad.norm() for p in plist])
        finite = torch.stack([torch.isfinite(p.grad).all() for p in plist])
        opt.step()
        seen.append((norms.cpu(), finite.cpu()))           # the one synchronisation a careful loop needs
        del seen[:-1]

    legs = [("a1", leg_a), ("t", leg_t), ("p", leg_p), ("a2", leg_a)]
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
    res["t_minus_a_ms"] = round(med["t"] - res["a_ms"], 4)
    res["p_minus_a_ms"] = round(med["p"] - res["a_ms"], 4)
    r = stats.read(wait=True)["grad"]
    res["step_tensors"] = len(r)
    res["step_nonfinite_tensors"] = len(stats.first_nonfinite())
    write(res, args.out)
    print(json.dumps(res, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
