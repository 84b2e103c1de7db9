"""What anchor clustering costs on the device (dyk_anchor_assign, dyk_anchor_median, dyk_anchor_fitness: csrc/anchors.hip) and
end to end (other_utils.anchor_cluster.k_means / evolve_anchors), beside the yardstick measured in the same run: the plain
numpy restatement tests/anchor_ref.py on the host CPU of the GPU machine (the yardstick, not the code under test).

Boxes: exp(RandomState(0).randn(N, 2) * 0.6 + 3.3) as float32, N = 2^16 and 2^20, K = 9.
  launches   each entry alone, its arguments on the device: back-to-back calls per leg and round between device events, as
             many as fill a window of `--window-ms` (20 ms; at least `iters`, counted from a first estimate and recorded as
             `calls_per_window`), legs alternating, median / min / max over `rounds` after a warm-up.  assign runs against
             its own previous result (changed = 0), median on the assignment of the k-means result, fitness with G = 64
             candidates.  `stats_readback_us`: the K + 2 counters copied to the host, 200 copies per window by the host clock,
             the device idle -- what k_means pays once per iteration beside its launches.
  fitness    divisions per second = 4 N K G over the median time (the fold launch included), and that rate times the 11 fp64
             VALU instructions one IEEE division expands to (counted in the ISA: 2 v_div_scale, v_rcp, 5 v_fma, v_mul,
             v_div_fmas, v_div_fixup) as a share of the vector fp64 issue rate (78.6 TFLOP/s in the public datasheet = 39.3 T
             lane-instructions/s; v_rcp_f64 and the division helpers issue slower than an FMA, so the share understates how busy
             the pipe is).  The boxes are read once per (item, candidate) from cache: 8 N G bytes against 4 N K G divisions.
  end_to_end k_means (np.random.seed(1)) and evolve_anchors(gen=1000, window=64; random.seed(2), np.random.seed(3)) from numpy
             boxes, host clock around the call (every call ends in a read-back), upload included; entry calls (k_means: one
             dyk_anchor_assign per iteration and one dyk_anchor_median per iteration but the last, the latter 10 launches and a
             memset in fp32 at K <= 16), fitness launches and read-backs as the wrappers count them; one warm-up call of each
             before, then `--e2e-runs` (5) timed runs with the same seeds: median / min / max of the seconds.
  numpy      the same two stages through tests/anchor_ref.py on the host CPU, one run each, same seeds; results compared bit
             for bit with the device's.  At N = 2^20 the sequential evolution is run for `--cpu-gen-large` generations only (20):
             its 1000-generation time is NOT measured, and the device result is compared over those generations.
Prints one JSON document; `--out FILE` also writes it.
usage: python tools/anchor_cluster_probe.py [--rounds 9] [--iters 20] [--window-ms 20] [--e2e-runs 5] [--out profiles/anchor_cluster.json]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

K, G, THR = 9, 64, 0.25
DIV_INSTRUCTIONS = 11                 # fp64 VALU instructions of one IEEE fp64 division (ISA of csrc/anchors.hip)
FP64_LANE_INSTR_PER_S = 78.6e12 / 2   # vector fp64 peak of the public datasheet, FMA = 2 FLOP


def stat(v, digits=2):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--cpu-gen-large", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("anchor_cluster_probe measures on the GPU; there is nothing to time without one")
    import anchor_ref as R
    from dyk import lib as L
    from dyk.buildinfo import native_sha
    from other_utils import anchor_cluster as A
    h = L.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    doc = {"code_sha": native_sha(), "device": torch.cuda.get_device_name(0), "K": K, "G": G, "thr": THR, "rounds": a.rounds, "min_iters": a.iters,
           "window_ms": a.window_ms, "e2e_runs": a.e2e_runs,
           "host_cpus_used_by_numpy": 1, "sizes": {}}
    for N in (int(s) for s in a.sizes.split(",")):
        wh = np.exp(np.random.RandomState(0).randn(N, 2) * 0.6 + 3.3).astype(np.float32)
        res = {}
        # ---- end to end on the device
        np.random.seed(1)
        A.k_means(wh, K)                                            # warm-up
        t_km, info = [], {}
        for _ in range(a.e2e_runs):
            np.random.seed(1)
            c, t = clock(lambda: A.k_means(wh, K, info=info))
            t_km.append(t)
        res["k_means"] = dict(info, seconds=stat(t_km, 4))
        k0 = c[np.argsort(c.prod(1))]
        A.evolve_anchors(wh, k0, thr=THR, gen=64)                   # warm-up
        t_ev, info = [], {}
        for _ in range(a.e2e_runs):
            random.seed(2)
            np.random.seed(3)
            (ke, fe, ne), t = clock(lambda: A.evolve_anchors(wh, k0, thr=THR, gen=1000, info=info))
            t_ev.append(t)
        res["evolve_anchors_gen1000"] = dict(info, seconds=stat(t_ev, 4), fitness_start=float(A.anchor_fitness(wh, k0, THR)[0]),
                                             fitness_end=float(fe))
        # ---- the launches alone
        dwh = torch.from_numpy(wh).cuda()
        dc = torch.from_numpy(c).cuda()
        nearest = torch.zeros(N, dtype=torch.int32, device="cuda")
        stats = torch.empty(K + 2, dtype=torch.int32, device="cuda")
        da = L.DykAnchorAssignDesc(wh=dwh.data_ptr(), c=dc.data_ptr(), nearest=nearest.data_ptr(), stats=stats.data_ptr(), N=N, K=K, elem_bytes=4)
        dc2 = dc.clone()
        mws = torch.empty(h.dyk_anchor_median_ws_bytes(K), dtype=torch.uint8, device="cuda")
        dm = L.DykAnchorMedianDesc(wh=dwh.data_ptr(), nearest=nearest.data_ptr(), c=dc2.data_ptr(), ws=mws.data_ptr(), ws_bytes=mws.numel(), N=N, K=K,
                                   elem_bytes=4)
        cand = torch.from_numpy((k0.astype(np.float64)[None] * R.draw_factors((K, 2), G)).clip(min=2.0)).cuda()
        need = h.dyk_anchor_fitness_ws_bytes(N, G, K)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.empty(24 * G, dtype=torch.uint8, device="cuda")
        p = out.data_ptr()
        df = L.DykAnchorFitnessDesc(wh=dwh.data_ptr(), a=cand.data_ptr(), ws=ws.data_ptr(), fit_boxes=p, fit_anchors=p + 8 * G, hit_boxes=p + 16 * G,
                                    hit_anchors=p + 20 * G, ws_bytes=need, thr=THR, N=N, K=K, G=G, elem_bytes=4)

        def leg(fn, d):
            def call():
                rc = fn(ctypes.byref(d), stream())
                assert rc == 0, rc
            return call
        legs = {"assign": leg(h.dyk_anchor_assign, da), "median": leg(h.dyk_anchor_median, dm), "fitness_G64": leg(h.dyk_anchor_fitness, df)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        calls = {k: min(5000, max(a.iters, int(a.window_ms * 1e3 / timed(fn, 5)) + 1)) for k, fn in legs.items()}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(timed(fn, calls[k]))
        res["launch_us"] = {k: dict(stat(v), calls_per_window=calls[k]) for k, v in times.items()}
        back = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(200):
                stats.cpu()
            back.append((time.perf_counter() - t) / 200 * 1e6)
        res["stats_readback_us"] = stat(back)
        divs = 4.0 * N * K * G
        per_s = divs / (res["launch_us"]["fitness_G64"]["median"] * 1e-6)
        res["fitness_fp64_divisions_per_s"] = float("%.4g" % per_s)
        res["fitness_share_of_fp64_vector_issue"] = round(per_s * DIV_INSTRUCTIONS / FP64_LANE_INSTR_PER_S, 3)
        res["fitness_bound_by"] = "fp64 VALU issue (divisions); memory traffic is 8 N G bytes from cache against 4 N K G divisions"
        # ---- the yardstick: numpy on this machine's CPU, same seeds
        np.random.seed(1)
        t = time.perf_counter()
        rc, iters, empties = R.k_means(wh, K)
        res["numpy_k_means"] = {"seconds": round(time.perf_counter() - t, 3), "iterations": iters, "empties": empties,
                                "equals_device_bit_for_bit": bool(np.array_equal(rc, c))}
        gen = 1000 if N <= 65536 else a.cpu_gen_large
        random.seed(2)
        np.random.seed(3)
        v = R.draw_factors((K, 2), 1000)
        t = time.perf_counter()
        rk, rf, rn = R.evolve(wh, k0, THR, gen, factors=v)
        t_ref = time.perf_counter() - t
        if gen == 1000:
            same = bool(np.array_equal(rk, ke) and rf == fe and rn == ne)
        else:
            random.seed(2)
            np.random.seed(3)
            kd, fd, nd = A.evolve_anchors(wh, k0, thr=THR, gen=gen)
            same = bool(np.array_equal(rk, kd) and rf == fd and rn == nd)
        res["numpy_evolve"] = {"generations": gen, "seconds": round(t_ref, 3), "seconds_per_generation": round(t_ref / max(gen, 1), 4),
                               "accepted": rn, "equals_device_bit_for_bit": same}
        doc["sizes"][str(N)] = res
        print("N=%d done" % N, file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
