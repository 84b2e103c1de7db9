"""bench_tuning.json is replayed by bench.py only when it was recorded for the kernel sources of the tree (its `native_sha`); otherwise
the benchmark tunes afresh and its outputs are no longer those of the recorded tiles.  A change to csrc/ that leaves the conv tile
choices valid re-stamps the file; one that does not re-records it (tools/record_bench_tuning.py)."""
import json
import os

from dyk.buildinfo import native_sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_recorded_tuning_is_for_the_sources_of_the_tree():
    with open(os.path.join(ROOT, "bench_tuning.json")) as f:
        rec = json.load(f)
    assert rec["native_sha"] == native_sha(), "bench_tuning.json was recorded for other kernel sources: bench.py would tune afresh"
    assert rec["choices"]
