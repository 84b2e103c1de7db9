"""Benchmark of the hot path named by BASELINE.json: paired RGB+LWIR images/s of a full train step
(forward + loss + backward + gradient all-reduce + optimizer) of Double-YOLOv4-Fshare-Global-CSE3
(kaist_dyolov4_fshare_global_concat_se3.cfg, 640x512, batch 16 per GPU, bf16 MFMA / fp32 accumulate).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0 (contract in the task statement): whole-job pairs/s and ms_per_step of the K timed
steps.  A plain run does only that.  With --full the line also carries
  "roofline"     for the dominant kernel (implicit-GEMM MFMA conv), measured live with HIP events
                 around every command of one extra profiling pass on the launch stream, and
  "cpu_baseline" the oracle (CPU restatement of the reference path) timed on the host cores on a
                 bounded sample (rank 0, N=1 only).
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (rank 0; see dump_outputs()).
Synthetic data per SURVEY.md §8(d): uint8 uniform paired images, 4 boxes per image, seeds 1234+rank.
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "double-yolo-kaist_amd")
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

CFG = "kaist_dyolov4_fshare_global_concat_se3"
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBPS = 8000.0         # HBM3E (MI355X_MICROARCH.md)
PROFILE_TAG = "r06"            # profiles/<tag>_*.json written by tools/run_gpu_round.sh for this round


def synth_batch(B, H, W, rank, device):
    g = torch.Generator().manual_seed(1234 + rank)
    v = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g)
    l = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g)
    nb = 4
    t = torch.zeros(B * nb, 6)
    t[:, 0] = torch.arange(B).repeat_interleave(nb).float()
    t[:, 2:4] = torch.rand(B * nb, 2, generator=g) * 0.8 + 0.1
    t[:, 4] = (torch.rand(B * nb, generator=g) * 60 + 16) / 640
    t[:, 5] = (torch.rand(B * nb, generator=g) * 120 + 32) / 512
    return v.to(device), l.to(device), t.to(device)


def load_hyp(img_size=512, nc=1):
    with open(os.path.join(PKG, "config", "hyp.scratch.4.json")) as f:
        hyp = json.load(f)
    hyp["cls"] *= nc / 80          # reference train.py:70-71
    hyp["obj"] *= img_size / 320
    return hyp


TUNING_FILE = os.path.join(ROOT, "bench_tuning.json")     # recorded tile choices of the benchmark's problems (tools/record_bench_tuning.py)
_PRIVATE = []


def private_dir():
    """one temporary directory per process, removed at exit: the benchmark writes nothing into the source tree, which may be
    read-only.  models.create_modules takes the head flavour from substrings of the cfg PATH ("yolov3", "yolov4", "fpn"),
    so the directory's own name must hold none of them."""
    if not _PRIVATE:
        import atexit
        import shutil
        import tempfile
        for _ in range(8):
            d = tempfile.mkdtemp(prefix="dyk-bench-")
            if not any(s in d for s in ("yolov", "fpn")):
                atexit.register(shutil.rmtree, d, True)
                _PRIVATE.append(d)
                break
            os.rmdir(d)
        else:
            sys.exit("bench.py: the temporary directory %s names a cfg flavour (yolov / fpn): set TMPDIR elsewhere" % d)
    return _PRIVATE[0]


def model_cfg(name):
    """config/<name>.cfg as materialize_cfg() writes it, but into private_dir()"""
    from build_utils.parse_config import materialize_cfg
    return materialize_cfg(name, out_dir=private_dir())


def use_recorded_tuning(device):
    """The autotuner times every candidate tile on the running chip and keeps the fastest; its measured durations also
    order the multi-stream schedule.  Two fresh processes can therefore choose differently, and a different summation
    order in bf16 grows over the timed training steps into outputs that differ by more than rounding.  So that the same
    arguments compute the same thing every run, the benchmark replays the choices recorded in bench_tuning.json -- the
    tuner's own cache format, loaded from a private copy -- when they were recorded for these kernel sources on this
    device.  Problems the table lacks (other cfgs / batches / dtypes) are tuned as usual.  Left alone when the caller
    steers the tuner (DYK_TUNE_CACHE, DYK_AUTOTUNE or a tuning switch).  Returns what was done, for stderr."""
    from dyk.buildinfo import native_sha
    from dyk.plan import _TUNE_KNOBS
    if "DYK_TUNE_CACHE" in os.environ or "DYK_AUTOTUNE" in os.environ or any(k.startswith(_TUNE_KNOBS) for k in os.environ):
        return "tuning as set by the environment"
    try:
        with open(TUNING_FILE) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return "no recorded tuning: tuning afresh"
    name = torch.cuda.get_device_name(device)
    if rec.get("native_sha") != native_sha() or rec.get("device") != name:
        return "recorded tuning is for %s on %s, this is %s on %s: tuning afresh" % (
            rec.get("native_sha"), rec.get("device"), native_sha(), name)
    path = os.path.join(private_dir(), "tune.json")
    with open(path, "w") as f:
        json.dump(rec["choices"], f)
    os.environ["DYK_TUNE_CACHE"] = path
    return "recorded tuning (%d problems)" % len(rec["choices"])


def conv_flops(plan, stems=True):
    """algorithmic conv flops of one forward pass of the plan: 2*B*Ho*Wo*Cout*Cin*k*k per [convolutional]
    (stems=False: without the Cin=3 stem layers, which run in their own direct kernel, not the implicit GEMM)"""
    total = 0.0
    for rec in plan.info:
        for r in (rec["parts"] if rec.get("kind") == "dwsep" else [rec]):
            if r.get("kind") != "conv" or (r["stem"] and not stems and "stem_direct" in r):
                continue
            z = r["z"]
            cin = 3 if r["stem"] else (1 if r["dw"] else r["x"].C)
            total += 2.0 * z.B * z.H * z.W * r["cout"] * cin * r["k"] * r["k"]
    return total


def layer_fused_floor(plan, es, peak_flops, bw):
    """SURVEY 8(d)(ii), literally: per [convolutional] layer of ONE pair's forward pass `max(flops_l / peak, bytes_l / BW)` with
    `bytes_l = elem_size * (|in| + |out| + |W|)` -- every layer fused with its BatchNorm / activation, every tensor crossing
    HBM once; a train step is 3 x B of it.  (C3: 150.7 us per pair = compute 85.7 / memory 129.1; the survey's probe: 150.9.)
    Also returns the share of the flops that sits in compute-bound layers: which roofline bounds the cfg."""
    tot = t_c = t_m = by_ = fl_ = fl_cb = 0.0
    for rec in plan.info:
        for r in (rec["parts"] if rec.get("kind") == "dwsep" else [rec]):
            if r.get("kind") != "conv":
                continue
            z, k, s = r["z"], r["k"], r["stride"]
            cin = 3 if r["stem"] else r["x"].C
            cin_g = 1 if r["dw"] else cin
            fl = 2.0 * z.H * z.W * r["cout"] * cin_g * k * k
            by = es * (z.H * s * z.W * s * cin + z.H * z.W * r["cout"] + r["cout"] * cin_g * k * k)
            tot += max(fl / peak_flops, by / bw)
            t_c += fl / peak_flops
            t_m += by / bw
            by_ += by
            fl_ += fl
            if fl / peak_flops > by / bw:
                fl_cb += fl
    return {"s_per_pair": tot, "compute_s": t_c, "memory_s": t_m, "bytes_per_pair": by_, "flops_per_pair": fl_,
            "compute_bound_flop_share": fl_cb / max(fl_, 1.0)}


def profile_plan(plan, stream, dump=None, cmds_out=None):
    """per-op-kind kernel time (ms) of one forward and one backward pass: every LAUNCH of the step -- the entries of
    the plan's schedule, two-problem launches of the twin sections included as the single launches they are -- timed
    alone on the chip with HIP events on `stream` (dyk_run_schedule_timed)"""
    from dyk import lib as L
    res = {}
    rows = []
    for which in ("fwd", "bwd"):
        cmds = plan.fwd if which == "fwd" else plan.bwd
        arr = plan._cfwd if which == "fwd" else plan._cbwd
        sc = plan.schedule(which, 0, len(cmds))
        ms = (ctypes.c_float * max(sc.n, 1))()
        L.check(L.load().dyk_run_schedule_timed(arr, sc.array, sc.n, ctypes.c_void_p(stream), ms), "dyk_run_schedule_timed")
        agg = {}
        base = len(cmds_out) if cmds_out is not None else 0
        for k, (e, t) in enumerate(zip(sc.entries, ms)):
            op, desc = cmds[e["cmd"]]
            nprob = 2 if e.get("cmd2", -1) >= 0 else 1
            a = agg.setdefault(op, [0, 0.0, 0])
            a[0] += 1
            a[1] += float(t)
            a[2] += nprob
            if cmds_out is not None:
                from cmd_roofline import cmd_model
                label, by, fl = cmd_model(L, op, desc, plan)
                cmds_out.append({"pass": which, "label": label + (" x2" if nprob == 2 else ""), "us": float(t) * 1e3,
                                 "bytes": by * nprob, "flops": fl * nprob, "deps": sc.entry_deps[k]})
            if dump is not None and op in (L.OP_CONV, L.OP_WGRAD):
                if op == L.OP_CONV:
                    rows.append(dict(pass_=which, op="conv", Cin=desc.Cin, Cout=desc.Cout, Hg=desc.Hg, Wg=desc.Wg, taps=desc.ntaps,
                                     isy=desc.isy, osy=desc.osy, flags=desc.flags, ms=float(t), problems=nprob,
                                     tflops=2.0 * nprob * desc.B * desc.Hg * desc.Wg * desc.Cin * desc.Cout * desc.ntaps / max(float(t), 1e-6) / 1e9))
                else:
                    ng = nprob * max(desc.group_n, 1)          # (a grouped launch carries group_n problems of this geometry)
                    rows.append(dict(pass_=which, op="wgrad", Cin=desc.Cin, Cout=desc.Cout, Hg=desc.Ho, Wg=desc.Wo, taps=desc.ntaps,
                                     isy=desc.isy, ms=float(t), problems=ng,
                                     tflops=2.0 * ng * desc.B * desc.Ho * desc.Wo * desc.Cin * desc.Cout * desc.ntaps / max(float(t), 1e-6) / 1e9))
        res[which] = agg
    if dump is not None:
        os.makedirs(os.path.dirname(dump), exist_ok=True)
        with open(dump, "w") as f:
            json.dump(rows, f)
    return res


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg_name, steps=2):
    """the oracle (CPU restatement of the reference path, plain torch CPU ops, parity-checked against the
    imported reference) on the host cores, bounded: (a) the BASELINE workload's cfg at batch 2, 512x640, full train step
    (forward + loss + backward), one untimed warm-up step then `steps` timed ones -> pairs/s, the unit of `value`;
    (b) config C1 exactly as BASELINE.json states it: kaist_yolov3.cfg, batch 2, 416x416, forward + loss."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from build_utils.parse_config import sections_from_json
    from oracle.model import OracleNet
    from oracle import loss as oloss
    cores = os.cpu_count() or 1
    # SURVEY 8(d) says "all host cores"; measured on the 256-thread GPU host (round 2): with all 256 threads this very
    # sample took 260 s per step (0.0077 pairs/s) -- the ~400 small CPU convolutions of a step only oversubscribe --
    # against ~1 pair/s on 32 threads.  The baseline is quoted at the setting that is fastest for the reference path.
    threads = int(os.environ.get("DYK_CPU_THREADS", min(cores, 32)))
    torch.set_num_threads(threads)
    hyp = load_hyp()

    def run(name, B, H, W, backward, n):
        net = OracleNet(sections_from_json(os.path.join(PKG, "config", "netdefs", name + ".json")), "config/%s.cfg" % name)
        sd = net.synth_state(0)
        if backward:
            for k, v in sd.items():
                if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")):
                    v.requires_grad_(True)
        v, l, t = synth_batch(B, H, W, 0, "cpu")
        av = net.anchor_vecs()
        dt = 0.0
        for i in range(n + 1):                       # step 0 = warm-up (first-call allocation / thread-pool start)
            t0 = time.time()
            with torch.set_grad_enabled(backward):
                p = net.forward(sd, v.float() / 255, l.float() / 255 if net.second_index is not None else None, training=True)
                ld = oloss.compute_loss(p, t, av, hyp, 1, 1.0, net.v4)
                if backward:
                    (ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]).backward()
            if i:
                dt += time.time() - t0
        return B * n / dt, dt

    c3, dt3 = run(cfg_name, 2, 512, 640, True, steps)
    c1, dt1 = run("kaist_yolov3", 2, 416, 416, False, 3)
    return {"value": c3, "unit": "pairs/s", "cores": threads, "kind": "port", "cpu": _cpu_model(), "host_cores": cores,
            "sample": "%d train steps (forward+loss+backward, fp32) of %s, batch 2, 512x640, after 1 warm-up step, oracle/ "
                      "(torch CPU ops) on %d threads, %.1f s" % (steps, cfg_name, threads, dt3),
            "c1": {"value": c1, "unit": "images/s", "sample": "kaist_yolov3.cfg batch 2, 416x416, forward + loss, 3 passes "
                   "after 1 warm-up, %.1f s" % dt1}}


DUMP_SAMPLE = 2_000_000        # elements kept of an output larger than this (fixed seeded sample, 8 MB in float32)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write each array as <out_dir>/<name>.npy in float32 (float64 stays float64).  An array of more than
    DUMP_SAMPLE elements is replaced by a fixed sample of its flattened values (seeded indices, ascending and distinct, the
    same for every run and build with the same shape), so that two builds can be compared output for output within 64 MB."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            g = torch.Generator().manual_seed(t.numel())
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=g).unique()
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))


def eval_bench(args):
    """inference pass of a cfg: forward + YOLO decode + non_max_suppression, batch images resident in HBM.
    Also times NMS alone on the dense worst case (every candidate survives, untrained weights) and on a
    trained-like synthetic prediction (~300 survivors per image)."""
    from build_utils.utils import non_max_suppression
    from models import YOLO
    device = torch.device("cuda", 0)
    print("bench.py:", use_recorded_tuning(device), file=sys.stderr)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = YOLO(model_cfg(args.cfg))
    model.dyk_dtype = args.dtype
    model = model.to(device).eval()
    B, H, W = args.batch, 512, 640
    v8, l8, _ = synth_batch(B, H, W, 0, device)

    def step(conf):
        with torch.no_grad():
            io, _ = model(v8.float() / 255.0, l8.float() / 255.0)
            return io, non_max_suppression(io, conf_thres=conf, iou_thres=0.6)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize()
        return (time.time() - t0) / n, r

    for _ in range(args.warmup):
        step(0.1)
    dt, (io, dets) = timed(lambda: step(0.1), args.steps)
    if args.dump_outputs:
        # the decoded heads and the NMS detections of the last timed step; detections as rows (image, x1, y1, x2, y2, conf, cls)
        rows = [torch.cat([torch.full((d.shape[0], 1), float(i), device=d.device), d.float()], 1)
                for i, d in enumerate(dets) if d is not None]
        dump_outputs(args.dump_outputs, {"io": io, "detections": torch.cat(rows) if rows else torch.zeros(0, 7)})
    nfwd, _ = timed(lambda: model(v8.float() / 255.0, l8.float() / 255.0), args.steps)
    ncand = int((io[..., 4] > 0.1).sum().item())
    dense = io.clone()
    dense[..., 4:] = dense[..., 4:].clamp(min=0.5)
    dense[..., 2:4] = dense[..., 2:4].clamp(3.0, 600.0)
    t_dense, _ = timed(lambda: non_max_suppression(dense, conf_thres=0.1, iou_thres=0.6), max(3, args.steps // 4))
    g = torch.Generator().manual_seed(3)
    sparse = dense.clone()
    keep = torch.rand(sparse.shape[:2], generator=g) < 300.0 / sparse.shape[1]
    sparse[..., 4] = torch.where(keep.to(device), sparse[..., 4], torch.full_like(sparse[..., 4], 0.01))
    t_sparse, _ = timed(lambda: non_max_suppression(sparse, conf_thres=0.1, iou_thres=0.6), args.steps)
    out = {"metric": "paired RGB+LWIR images/sec (eval: forward + decode + NMS)", "value": B / dt, "unit": "pairs/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": "%s.cfg eval forward + decode + NMS, 640x512 pairs, batch %d" % (args.cfg, B)},
           "forward_ms": nfwd * 1e3, "candidates_over_conf": ncand,
           "nms": {"rows_per_image": int(io.shape[1]),
                   "dense_all_survive": {"ms_per_batch": t_dense * 1e3, "images_per_s": B / t_dense, "candidates_per_s": B * io.shape[1] / t_dense},
                   "sparse_300_survivors": {"ms_per_batch": t_sparse * 1e3, "images_per_s": B / t_sparse}}}
    # AP of the 64-pair trained-head fixture on both arithmetic paths, as measured by tests/test_eval_ap.py on the running
    # code (the test writes profiles/<tag>_ap_64pair.json through DYK_AP_JSON; reported only when its code hash matches)
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from code_sha import code_sha
        aj = {}
        for cand in (os.path.join(ROOT, "profiles", PROFILE_TAG + "_ap_64pair.json"), os.path.join(ROOT, "gpurun_out", "ap_64pair.json")):
            if os.path.exists(cand):
                with open(cand) as f:
                    aj = json.load(f)
                if aj.get("code_sha") == code_sha():
                    break
        if aj.get("code_sha") == code_sha() and "fp32" in aj and "bf16" in aj:
            out["ap_64pair"] = {"reference_fp32": aj["reference"], "hip_fp32": aj["fp32"]["ap"], "hip_bf16": aj["bf16"]["ap"],
                                "bf16_minus_fp32_ap_points": 100.0 * (aj["bf16"]["ap"] - aj["fp32"]["ap"]),
                                "bf16_emulating_oracle": aj["bf16"].get("emulated_ap"),
                                "this_line_dtype": args.dtype,
                                "source": "%s (tests/test_eval_ap.py on this code)" % os.path.relpath(cand, ROOT)}
    except Exception:
        pass
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="per-GPU batch (pairs)")
    ap.add_argument("--cfg", default=CFG)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the roofline pass and the CPU baseline (off: the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline pass")
    ap.add_argument("--dump-layers", default=None, help="with --full: write per-conv-launch timings to this JSON file")
    ap.add_argument("--dump-cmds", default=None, help="with --full: write every command's isolated time + algorithmic bytes / "
                                                      "flops to this JSON file (tools/cmd_roofline.py reads it)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float32, seeded samples of large arrays)")
    ap.add_argument("--mode", default="train", choices=["train", "eval"],
                    help="train: the BASELINE metric (default).  eval: forward + decode + NMS of --cfg (SURVEY 8d, config C2)")
    args = ap.parse_args()
    if (args.dump_layers or args.dump_cmds) and not (args.full and not args.no_roofline and args.mode == "train"):
        ap.error("--dump-layers / --dump-cmds come from the roofline pass: they need --full (train mode, without --no-roofline)")
    if args.mode == "eval":
        return eval_bench(args)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start one rank per GPU over RCCL (the driver's torchrun form sets
        # WORLD_SIZE itself and lands in the branch below)
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.exit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (args.gpus, have))
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=env))

    # the ONE JSON line must be the last thing on stdout: RCCL / HIP libraries write banners through C stdio (flushed at
    # exit, i.e. after Python's own output), so fd 1 is pointed at stderr and the JSON goes out through a private handle
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and not os.environ.get("DYK_FORCE_DDP"):
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1 or os.environ.get("DYK_FORCE_DDP"):       # DYK_FORCE_DDP=1: exercise the exchange path on one GPU
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local)
        # NO `device_id=`: binding the process group to the device at init (eager communicator) costs the step 3.3 ms on
        # this stack (PyTorch 2.10 + ROCm 7.0: 39.2 vs 36.1 ms with NOTHING else changed, no collective in the step) --
        # measured in-call; the communicator is created by the warm-up collective below instead
        dist.init_process_group("nccl")
        dist.all_reduce(torch.ones(8, device=torch.device("cuda", local)))
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)

    from build_utils.utils import compute_loss
    from dyk.ddp import GradAllReduce, reduce_dict
    from dyk.optim import FusedAdam
    from models import YOLO

    print("bench.py:", use_recorded_tuning(device), file=sys.stderr)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):          # the reference-style "Model Summary" line is not bench output
        model = YOLO(model_cfg(args.cfg))
    model.nc, model.hyp, model.gr = 1, load_hyp(), 1.0
    model.dyk_dtype = args.dtype
    model = model.to(device).train()
    hyp = model.hyp
    B, H, W = args.batch, 512, 640
    v8, l8, targets = synth_batch(B, H, W, rank, device)
    opt = FusedAdam(model, lr=hyp["lr0"], betas=(hyp["momentum"], 0.999), weight_decay=hyp["weight_decay"])
    reducer = GradAllReduce(model, dist) if dist is not None else None
    if reducer is not None:
        opt.grad_scale = 1.0 / world

    # first-epoch linear learning-rate warm-up of the reference harness (kaist_train_eval_utils.py:28-35,
    # distributed_utils.py warmup_lr_scheduler: factor 1/1000 -> 1 over 1000 iterations).  On uniform-noise
    # images a cold start at lr0 drives box sizes to 0 within a few steps, where the CIoU term atan(w/h) has
    # a 0*inf gradient in the reference's own math (and here) -- the warm-up is what the reference trains with.
    it = [0]
    host_tl = bool(os.environ.get("DYK_HOST_TIMELINE"))
    float_input = bool(os.environ.get("DYK_BENCH_FLOAT_INPUT"))     # analysis: when does the host return from each phase

    phase_ev = [] if os.environ.get("DYK_PHASE_EVENTS") else None   # analysis: GPU-side span of each phase (events, no host sync)

    def mark(row):
        if row is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            row.append(e)

    def step():
        row = None
        if phase_ev is not None:
            row = []
            phase_ev.append(row)
            mark(row)
        alpha = min(it[0] / 1000.0, 1.0)
        opt.param_groups[0]["lr"] = hyp["lr0"] * (0.001 * (1 - alpha) + alpha)
        it[0] += 1
        tl = [time.perf_counter()] if host_tl else None
        # the loader's uint8 batches go in as they are: the `.float() / 255.0` of kaist_train_eval_utils.py:54-55 is done
        # inside the stem kernel (same fp32 quotient), still inside the timed step (DYK_BENCH_FLOAT_INPUT=1: outside)
        if float_input:
            pred = model(v8.float() / 255.0, l8.float() / 255.0)
        else:
            pred = model(v8, l8)
        mark(row)
        if host_tl: tl.append(time.perf_counter())
        ld = compute_loss(pred, targets, model)
        loss = ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]
        mark(row)
        if host_tl: tl.append(time.perf_counter())
        if reducer is not None:
            reduce_dict(ld)                          # the harness's per-step loss exchange (kaist_train_eval_utils.py:82)
        loss.backward()
        mark(row)
        if host_tl: tl.append(time.perf_counter())
        if reducer is not None:
            reducer.all_reduce(optimizer=opt)        # step() updates each bucket's range behind its own all-reduce (dyk/ddp.py)
        opt.step()
        mark(row)
        if host_tl:
            tl.append(time.perf_counter())
            torch.cuda.synchronize()
            tl.append(time.perf_counter())
            print("host timeline ms: fwd %.2f loss %.2f bwd %.2f opt %.2f | gpu drained at %.2f" % tuple(
                (b - tl[0]) * 1e3 for b in tl[1:]), file=sys.stderr)
        return loss, pred, ld

    for _ in range(args.warmup):
        loss, pred, ld = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    # per-step durations from HIP events on the step's stream (no host synchronisation inside the timed region): median_ms
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    evs[0].record()
    for q in range(args.steps):
        loss, pred, ld = step()
        evs[q + 1].record()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.time() - t0
    if phase_ev:
        rows = [r for r in phase_ev[-args.steps:] if len(r) == 5]
        spans = [sum(r[k].elapsed_time(r[k + 1]) for r in rows) / len(rows) for k in range(4)]
        print("GPU phase spans ms (stream-ordered events, mean of %d steps): forward %.3f | loss %.3f | backward %.3f | optimizer %.3f"
              % ((len(rows),) + tuple(spans)), file=sys.stderr)
    rccl_ranks = None
    if dist is not None:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        # proof that the collective saw every rank: a SUM of ones over the job's communicator
        one = torch.ones(1, device=device, dtype=torch.float64)
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        rccl_ranks = int(round(float(one.item())))
    final_loss = float(loss.item())
    if rank == 0 and args.dump_outputs:
        # what a caller of the train step receives from its last timed run: the three heads' raw predictions, the loss terms
        # and the parameters after the optimizer step (in model.parameters() order; written before the --full profiling pass,
        # which reruns the plan's commands)
        params = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        bufs = torch.cat([b.detach().reshape(-1).float() for b in model.buffers() if b.dtype.is_floating_point])
        arrays = {"pred_%d" % i: p for i, p in enumerate(pred)}
        arrays.update({"loss": torch.stack([loss.reshape(()), ld["box_loss"].reshape(()), ld["obj_loss"].reshape(()),
                                            ld["class_loss"].reshape(())]),
                       "params_after_step": params, "bn_running_stats": bufs})
        dump_outputs(args.dump_outputs, arrays)
        del params, bufs, arrays

    out = None
    if rank == 0:
        ms = dt / args.steps * 1e3
        pairs = B * world * args.steps / dt
        out = {"metric": "paired RGB+LWIR images/sec (train step)", "value": pairs, "unit": "pairs/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "%s.cfg train step (fwd+loss+bwd+Adam%s), 640x512 pairs, batch %d/GPU"
                                      % (args.cfg, "+RCCL grad all-reduce" if world > 1 else "", B),
                          "global_batch": B * world, "parallelism": "dp%d" % world},
               "final_loss": final_loss, "rccl_ranks": rccl_ranks,
               "median_ms": sorted(evs[q].elapsed_time(evs[q + 1]) for q in range(args.steps))[args.steps // 2]}
        if args.full and not args.no_roofline:
            plan = model.engine.plans[(B, H, W, torch.bfloat16 if args.dtype == "bf16" else torch.float32, True)]
            from dyk import lib as L
            cmds_out = [] if args.dump_cmds else None
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            prof = profile_plan(plan, torch.cuda.current_stream().cuda_stream, args.dump_layers, cmds_out)
            if cmds_out is not None:
                # (rows carry their dependency lists -- launch positions within the pass -- for the critical-path figure
                # of tools/cmd_roofline.py)
                with open(args.dump_cmds, "w") as f:
                    json.dump(cmds_out, f)
            f1_all = conv_flops(plan)
            f1 = conv_flops(plan, stems=False)          # what the implicit-GEMM family computes
            ig_ms = prof["fwd"].get(L.OP_CONV, [0, 0.0, 0])[1] + prof["bwd"].get(L.OP_CONV, [0, 0.0, 0])[1]
            ig_n = prof["fwd"].get(L.OP_CONV, [0, 0.0, 0])[0] + prof["bwd"].get(L.OP_CONV, [0, 0.0, 0])[0]
            wg_n, wg_ms = prof["bwd"].get(L.OP_WGRAD, [0, 0.0, 0])[:2]
            peak = PEAK_BF16_TFLOPS if args.dtype == "bf16" else PEAK_F32_TFLOPS
            ach = 2.0 * f1 / (ig_ms * 1e-3) / 1e12 if ig_ms > 0 else 0.0      # forward + data-gradient launches
            tot_ms = sum(a[1] for w in prof.values() for a in w.values())
            es = 2 if args.dtype == "bf16" else 4
            peak_f = peak * 1e12
            # composite roofline per LAYER-FUSED pass (every layer's in + out + W once) -- `composite_roofline`;
            # beside it, under its own name, the floor of the launches this design actually makes (every command's own
            # algorithmic bytes / flops, i.e. the separate BatchNorm passes counted as work): `per_command_floor`
            lf = layer_fused_floor(plan, es, peak_f, PEAK_HBM_GBPS * 1e9)
            lf_ms = lf["s_per_pair"] * 3.0 * B * 1e3
            comp = {"floor_ms": lf_ms, "frac": lf_ms / ms,
                    "definition": "SURVEY 8d(ii): sum over layers of max(flops/peak, es*(|in|+|out|+|W|)/8 TB/s) of one pair's forward "
                                  "x 3 x B / t_step", "per_pair_fwd_us": lf["s_per_pair"] * 1e6,
                    "compute_us": lf["compute_s"] * 1e6, "memory_us": lf["memory_s"] * 1e6,
                    "bytes_per_pair_fwd": lf["bytes_per_pair"], "compute_bound_flop_share": lf["compute_bound_flop_share"]}
            per_cmd = None
            try:
                from cmd_roofline import cmd_model
                fl_ms = 0.0
                for which in ("fwd", "bwd"):
                    for op, desc in (plan.fwd if which == "fwd" else plan.bwd):
                        _, by, fl = cmd_model(L, op, desc, plan)
                        fl_ms += max(by / (PEAK_HBM_GBPS * 1e9), fl / peak_f) * 1e3
                per_cmd = {"floor_ms": fl_ms, "frac": fl_ms / ms,
                           "definition": "sum over the step's COMMANDS of max(bytes/8 TB/s, flops/peak) / t_step: the floor of the "
                                         "launches as designed (separate BatchNorm passes count as work); not SURVEY 8d(ii)"}
            except Exception:
                pass
            # which roofline bounds the cfg: MFMA when most of its flops sit in layers whose flop time exceeds their byte time
            # (C3: the 3x3 convs, 84 % of the flops), HBM otherwise (the MobileNet cfgs: SURVEY 8d "(ii) with HBM only")
            hbm_bound = lf["compute_bound_flop_share"] < 0.5
            # HBM-side bytes per launch and the IN-STEP durations of the same kernels come from rocprofv3 runs of this very
            # command (tools/run_gpu_round.sh -> profiles/): they are reported only when those files were produced by
            # the code that is running now (hash over the kernel sources and the plan compiler), otherwise null
            FAM = ("conv_igemm_kernel", "conv_halo_kernel", "conv_lt_kernel", "conv_sc_kernel", "conv_pw_kernel")
            traffic, in_step, src, step_hbm = None, None, None, None
            is_headline = args.cfg == CFG and B == 16 and args.dtype == "bf16"     # what profiles/<tag>_* were taken on
            try:
                from code_sha import code_sha
                sha = code_sha()
                with open(os.path.join(ROOT, "profiles", PROFILE_TAG + "_pmc_summary.json")) as f:
                    pj = json.load(f)
                if pj.get("code_sha") == sha and is_headline:
                    ks = [pj["kernels"][k] for k in FAM if k in pj["kernels"]]
                    # family-wide, the same base as `launches` / `flops_per_launch` below
                    traffic = sum(k_["fetch_bytes"] + k_["write_bytes"] for k_ in ks) / max(sum(k_["dispatches"] for k_ in ks), 1)
                    step_hbm = pj.get("step_hbm_bytes")
                    src = "profiles/%s_pmc_summary.json" % PROFILE_TAG
                with open(os.path.join(ROOT, "profiles", PROFILE_TAG + "_step_kernels.json")) as f:
                    kj = json.load(f)
                if kj.get("code_sha") == sha and is_headline:
                    fams = [kj["families"][k] for k in FAM if k in kj["families"]]
                    t_us = sum(f_["total_us"] for f_ in fams)
                    in_step = {"tflops": 2.0 * f1 / (t_us * 1e-6) / 1e12, "frac": 2.0 * f1 / (t_us * 1e-6) / 1e12 / peak,
                               "launches": sum(f_["n"] for f_ in fams), "total_us": t_us,
                               "avg_launch_us": t_us / max(sum(f_["n"] for f_ in fams), 1),
                               "source": "profiles/%s_step_kernels.json (rocprofv3 kernel trace of one step; four streams run "
                                         "concurrently, so a launch's duration includes the time it shares the chip: the summed "
                                         "durations exceed the step)" % PROFILE_TAG}
            except Exception:
                pass
            alg_bytes_launch = None
            try:
                from cmd_roofline import cmd_model
                ab = sum(cmd_model(L, op, desc, plan)[1] for which in ("fwd", "bwd")
                         for op, desc in (plan.fwd if which == "fwd" else plan.bwd) if op == L.OP_CONV)
                alg_bytes_launch = ab / max(ig_n, 1)
            except Exception:
                pass
            detail = {
                "conv_fwd_flops_per_step": f1_all, "igemm_fwd_flops_per_step": f1,
                "wgrad_tflops": (f1 / (wg_ms * 1e-3) / 1e12) if wg_ms > 0 else 0.0, "wgrad_ms": wg_ms, "wgrad_launches": wg_n,
                "igemm_ms": ig_ms, "all_kernels_ms": tot_ms,
                "step_mfma_frac": 3.0 * f1_all / (ms * 1e-3) / 1e12 / peak,
                "step_hbm_frac": lf["bytes_per_pair"] * 3.0 * B / (ms * 1e-3) / (PEAK_HBM_GBPS * 1e9),
                "composite_roofline": comp, "per_command_floor": per_cmd,
                "step_hbm_bytes_pmc": step_hbm,
                "launches_per_step": sum(a[0] for w in prof.values() for a in w.values()),
                "commands_per_step": sum(a[2] for w in prof.values() for a in w.values()),
                "per_op_ms": {w: {str(k): [a[0], round(a[1], 4)] for k, a in prof[w].items()} for w in prof}}
            if hbm_bound:
                # "For C5 the figure is (ii) with HBM only: achieved_GBps = bytes_per_pair x 3 x B / t_step vs 8 TB/s"
                gbps = lf["bytes_per_pair"] * 3.0 * B / (ms * 1e-3) / 1e9
                out["roofline"] = {
                    "bound": "hbm", "kernel": "whole step (the cfg's layers are HBM-bound: %.0f %% of its flops sit in compute-bound "
                                              "layers)" % (100 * lf["compute_bound_flop_share"]),
                    "achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": gbps / PEAK_HBM_GBPS,
                    "traffic": step_hbm, "traffic_unit": "HBM bytes per step (rocprofv3 PMC)" if step_hbm else None,
                    "frac_is": "layer-fused algorithmic bytes of a train step (3 x B x %.1f MB) over the measured step time"
                               % (lf["bytes_per_pair"] / 1e6),
                    "conv_family_mfma": {"achieved_isolated": ach, "frac_isolated": ach / peak, "launches": ig_n},
                    "detail": detail}
            else:
                # `achieved` / `frac`: measured in THIS run -- every launch of the family timed alone with HIP events on the launch
                # stream right after the timed steps (dyk_run_schedule_timed).  `in_step` is the rocprofv3 figure of the same
                # launches while four streams share the chip (only when profiles/ holds a trace of the running code).
                out["roofline"] = {
                    "bound": "mfma", "kernel": "conv_igemm_kernel + conv_lt_kernel + conv_halo_kernel + conv_sc_kernel + conv_pw_kernel (forward + data-gradient launches)",
                    "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                    "traffic": traffic,
                    "traffic_unit": "HBM bytes per launch, family-wide (rocprofv3 PMC, %s)" % src if src else None,
                    "algorithmic_bytes_per_launch": alg_bytes_launch,
                    "frac_is": "every launch of the family timed ALONE with HIP events on its launch stream, in this run "
                               "(profiles/%s_serial_kernels.txt: rocprofv3 --stats of the same plan on one stream); `in_step`: the "
                               "same launches inside the four-stream step" % PROFILE_TAG,
                    "frac_isolated": ach / peak, "achieved_isolated": ach,
                    "frac_in_step": in_step["frac"] if in_step else None,
                    "in_step": in_step,
                    "launches": ig_n, "avg_launch_ms": ig_ms / max(ig_n, 1),
                    "flops_per_launch": 2.0 * f1 / max(ig_n, 1),
                    "detail": detail}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cfg)
        json_out.write(json.dumps(out) + "\n")
        json_out.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
