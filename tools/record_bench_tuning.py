"""Record the autotuner's tile choices for bench.py's default workload -- the train step and `--mode eval` of the target
cfg, batch 16, bf16 -- into bench_tuning.json, which bench.py replays so that its runs compute the same thing every time
(bench.py: use_recorded_tuning).  Run on an MI355X after build(), whenever the kernel sources change (the table names the
source digest it belongs to and is ignored otherwise):

    python tools/record_bench_tuning.py [OUT]        (default: bench_tuning.json in the repository root)
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "double-yolo-kaist_amd")
sys.path[:0] = [ROOT, PKG]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "bench_tuning.json")
    from dyk.buildinfo import native_sha
    from dyk.plan import _TUNE_KNOBS
    steer = sorted(k for k in os.environ if k.startswith(_TUNE_KNOBS) or k in ("DYK_TUNE_CACHE", "DYK_AUTOTUNE"))
    if steer:
        sys.exit("record_bench_tuning.py: unset %s first (the table is for the default tuner)" % " ".join(steer))
    with tempfile.TemporaryDirectory() as d:
        cache = os.path.join(d, "tune.json")
        env = dict(os.environ, DYK_TUNE_CACHE=cache)
        for mode in ("train", "eval"):
            # a fresh process per mode (the tuner runs at the first step); both merge into the same cache file
            subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", mode, "--steps", "2", "--warmup", "1"],
                           env=env, check=True, stdout=subprocess.DEVNULL)
        with open(cache) as f:
            choices = json.load(f)
    import torch
    rec = {"native_sha": native_sha(), "device": torch.cuda.get_device_name(0), "choices": choices}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d problems, sources %s, %s" % (out, len(choices), rec["native_sha"], rec["device"]))


if __name__ == "__main__":
    main()
