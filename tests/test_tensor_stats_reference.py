"""Per-tensor statistics (csrc/tensor_stats.hip, dyk/monitor.py) on the CPU: the work list, the numpy restatement of the
documented addition order (tests/tensor_stats_ref.py) against the plain fp64 reference and the bound derived there, a list of
wrong kernels that the named cases must flag, ParamStore.segment_table() against the model, the layouts of the new structures
against gcc and the argument refusals of dyk_tensor_stats that need no GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import tensor_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ work list
def _random_table(rng):
    segs, off = [], int(rng.integers(0, 4)) * 4
    for _ in range(int(rng.integers(1, 40))):
        numel = int(rng.choice([1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8192, int(rng.integers(1, 20000))]))
        segs.append((off, numel, int(rng.integers(0, 16))))
        off += numel
        off = (off + 3) // 4 * 4 + int(rng.integers(0, 3)) * 4 if rng.integers(0, 2) else (off + 63) // 64 * 64
    return segs


@pytest.mark.parametrize("seed", range(8))
def test_work_list_partitions_every_segment(seed):
    from dyk import ops
    table = _random_table(np.random.default_rng(seed))
    segs, items = R.work_list(table)
    covered = {}
    for i, it in enumerate(items):
        s, first, ln = int(it["seg"]), int(it["first"]), int(it["len"])
        off, numel, _ = table[s]
        assert 1 <= ln <= R.ITEM
        assert off <= first and first + ln <= off + numel, "item %d crosses its segment" % i
        assert first % 4 == 0
        covered.setdefault(s, []).append((first, ln))
    assert sorted(covered) == list(range(len(table))), "a segment without items"
    assert list(items["seg"]) == sorted(items["seg"]), "items are not in segment order"
    for s, (off, numel, flags) in enumerate(table):
        spans = covered[s]
        assert spans == sorted(spans)
        assert spans[0][0] == off and sum(ln for _, ln in spans) == numel
        assert all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])), "a gap or an overlap inside segment %d" % s
        assert all(ln == R.ITEM for _, ln in spans[:-1])
        assert int(segs[s]["item_begin"]) == int(np.flatnonzero(items["seg"] == s)[0]) and int(segs[s]["flags"]) == flags
        assert len(spans) == R.items_of(numel)
    # the builder the product uses gives the same bytes
    psegs, pitems = ops.tensor_stats_tables(table)
    assert psegs.tobytes() == segs.tobytes() and pitems.tobytes() == items.tobytes()
    assert psegs.dtype.itemsize == 24 and pitems.dtype.itemsize == 16


def test_table_builder_refuses_what_the_kernel_does_not_take():
    from dyk import ops
    for bad in ([], [(2, 8, 0)], [(0, 0, 0)], [(-4, 8, 0)], [(0, 8, 16)]):
        with pytest.raises(ValueError):
            ops.tensor_stats_tables(bad)


# ------------------------------------------------------------------ the restatement against the plain reference
@pytest.mark.parametrize("style,nbuf,specials,skips", [("store", 1, False, False), ("packed", 2, True, False),
                                                       ("mixed", 4, True, True), ("mixed", 3, False, True)])
def test_restatement_stays_inside_the_bound(style, nbuf, specials, skips):
    bufs, segments = R.kernel_case(style, nbuf, specials, skips)
    rec = R.restate(bufs, segments)
    assert R.deviations(rec, bufs, segments) == []
    # ... and against the exact sum, with the bound of the device's order alone; np.sum stays inside its own allowance
    for s, (off, numel, flags) in enumerate(segments):
        for k, b in enumerate(bufs):
            if (flags >> k) & 1:
                continue
            exact = R.exact_sumsq(b[off:off + numel])
            assert abs(float(rec[s, k]["sumsq"]) - exact) <= (R.sumsq_bound(numel) + R.U) * exact
            x = b[off:off + numel]
            xd = x[np.abs(x) <= np.float32(R.F32_MAX)].astype(np.float64)
            assert abs(float(np.sum(xd * xd)) - exact) <= (R.gamma(R.pairwise_roundings(numel)) + R.U) * exact


def test_bound_constants():
    assert R.roundings(1) == 32 and R.roundings(512 * 1024 * 9) == 49
    worst = 2 ** 28
    assert R.norm_bound(worst) + 2.0 ** -24 < 2.0 ** -23
    assert R.other_order_bound(worst - 1) + 2.0 ** -24 < 2.0 ** -23


def test_a_large_segment_uses_every_fold_lane_more_than_once():
    """70 items: fold lanes 0..5 add two partials; values of one magnitude so that every rounding counts"""
    numel = 69 * R.ITEM + 77
    rng = np.random.default_rng(11)
    buf = np.full(numel + 72, np.nan, np.float32)
    buf[8:8 + numel] = (1.0 + rng.random(numel)).astype(np.float32)
    segments = [(8, numel, 0)]
    rec = R.restate([buf], segments)
    assert R.deviations(rec, [buf], segments) == []
    exact = R.exact_sumsq(buf[8:8 + numel])
    assert abs(float(rec[0, 0]["sumsq"]) - exact) <= (R.sumsq_bound(numel) + R.U) * exact


# ------------------------------------------------------------------ wrong kernels
@pytest.mark.parametrize("wrong", R.WRONG_KERNELS)
def test_wrong_kernels_are_flagged(wrong):
    cases = R.wrong_kernel_cases()
    assert sorted(cases) == sorted(R.WRONG_KERNELS)
    bufs, segments = cases[wrong]
    assert R.deviations(R.restate(bufs, segments), bufs, segments) == [], "the right kernel fails the case"
    found = R.deviations(R.restate(bufs, segments, wrong=wrong), bufs, segments)
    print(wrong, "->", found[:3])
    assert found, "the case does not flag the wrong kernel %r" % wrong


def test_every_wrong_kernel_is_flagged_by_the_gpu_cases_too():
    """the synthetic tables of tests/test_gpu_tensor_stats.py, taken together, tell every wrong kernel from the right one"""
    left = set(R.WRONG_KERNELS)
    for style, nbuf, specials, skips in (("mixed", 2, True, True), ("packed", 1, True, False)):
        bufs, segments = R.kernel_case(style, nbuf, specials, skips)
        for w in sorted(left):
            if R.deviations(R.restate(bufs, segments, wrong=w), bufs, segments):
                left.discard(w)
    assert left <= {"padding_in_zeros"}, left          # (NaN padding cannot show that one: its own case above does)


# ------------------------------------------------------------------ the store's table
def test_segment_table_of_a_model():
    from build_utils.parse_config import materialize_cfg
    from models import YOLO
    m = YOLO(materialize_cfg("kaist_yolov3"))
    st = m.engine.store
    params, running = st.segment_table()
    named = [n for n, _ in m.named_parameters()]
    assert [n for n, _, _ in params] == named
    assert [(o, n) for _, o, n in params] == [(e.offset, e.numel) for e in st.entries]
    assert [n for _, _, n in params] == [p.numel() for _, p in m.named_parameters()]
    assert all(o % 64 == 0 for _, o, _ in params)
    buffers = dict(m.named_buffers())
    assert [n for n, _, _ in running] == [n for n in buffers if n.endswith(("running_mean", "running_var"))]
    assert [(o, n) for _, o, n in running] == [(o, n) for _, _, o, n in st.rstats]
    assert all(buffers[name].numel() == n for name, _, n in running)
    # the segments of a table do not overlap and stay inside the flat buffer
    for tab, total in ((params, st.total), (running, st.rtotal)):
        ends = [o + n for _, o, n in tab]
        assert all(e <= o for e, (_, o, _) in zip(ends, tab[1:])) and ends[-1] <= total


def test_tensor_stats_arguments():
    from build_utils.parse_config import materialize_cfg
    from dyk.monitor import TensorStats
    from dyk.optim import FusedAdam, FusedSGD
    from models import YOLO
    m = YOLO(materialize_cfg("kaist_yolov3"))
    for bad in ((), ("gradient",), ("grad", "grad")):
        with pytest.raises(ValueError):
            TensorStats(m, what=bad)
    with pytest.raises(ValueError, match="optimizer"):
        TensorStats(m, what=("exp_avg",))
    with pytest.raises(ValueError, match="keeps no"):
        TensorStats(m, what=("momentum",), optimizer=FusedAdam(m))
    with pytest.raises(ValueError, match="keeps no"):
        TensorStats(m, what=("exp_avg_sq",), optimizer=FusedSGD(m))
    other = YOLO(materialize_cfg("kaist_yolov3"))
    with pytest.raises(ValueError, match="of this model"):
        TensorStats(m, what=("exp_avg",), optimizer=FusedAdam(other))
    ts = TensorStats(m, what=("param", "grad", "exp_avg", "exp_avg_sq", "running"), optimizer=FusedAdam(m))
    assert ts.read() is None and ts.first_nonfinite(wait=False) == [] and "nothing" in ts.summary()
    from dyk import lib
    with pytest.raises(lib.DykError):
        ts.launch()                      # no forward pass yet: the store is not on a device


# ------------------------------------------------------------------ ABI
NEW_STRUCTS = ["DykTensorSeg", "DykTensorItem", "DykTensorStat", "DykTensorStatsDesc"]


def test_new_struct_layouts_match_the_c_compiler(tmp_path):
    from dyk import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){"]
    for s in NEW_STRUCTS:
        lines.append('printf("%s %%zu %%zu\\n", sizeof(%s), _Alignof(%s));' % (s, s, s))
        for f, _ in getattr(lib, s)._fields_:
            lines.append('printf("%s.%s %%zu 0\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append('printf("MAX_BUFS %d 0\\nITEM %d 0\\n", DYK_TSTAT_MAX_BUFS, DYK_TSTAT_ITEM);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in subprocess.check_output([str(exe)]).decode().splitlines()}
    for s in NEW_STRUCTS:
        cls = getattr(lib, s)
        assert out[s] == (ctypes.sizeof(cls), ctypes.alignment(cls)), s
        for f, _ in cls._fields_:
            assert out["%s.%s" % (s, f)][0] == getattr(cls, f).offset, (s, f)
    assert out["DykTensorStat"] == (24, 8)
    assert out["MAX_BUFS"][0] == lib.TSTAT_MAX_BUFS and out["ITEM"][0] == lib.TSTAT_ITEM == R.ITEM
    assert (R.SEG.itemsize, R.ITEM_T.itemsize, R.STAT.itemsize) == (24, 16, 24)
    for dt, s in ((R.SEG, "DykTensorSeg"), (R.ITEM_T, "DykTensorItem"), (R.STAT, "DykTensorStat")):
        for f, _ in getattr(lib, s)._fields_:
            assert dt.fields[f][1] == getattr(getattr(lib, s), f).offset


def _desc(lib, **kw):
    """a descriptor whose every check passes (addresses are never dereferenced by a refused call) with `kw` written over it"""
    d = lib.DykTensorStatsDesc()
    for k in range(4):
        d.buf[k] = 0x1000 * (k + 1)
    d.seg, d.items, d.ws, d.out = 0x10000, 0x20000, 0x30000, 0x40000
    d.n, d.nbuf, d.nseg, d.nitems = 4096, 2, 3, 5
    d.ws_bytes = 24 * 5 * 2
    for k, v in kw.items():
        if k.startswith("buf"):
            d.buf[int(k[3:])] = v
        else:
            setattr(d, k, v)
    return d


def test_arguments_are_refused_before_any_launch():
    from dyk import lib
    h = lib.load()
    assert h.dyk_abi_version() == 5
    assert h.dyk_tensor_stats(None, None) == -1
    assert h.dyk_tensor_stats_ws_bytes(5, 2) == 240 and h.dyk_tensor_stats_ws_bytes(1152, 4) == 1152 * 96
    for items, nbuf in ((0, 1), (-1, 1), (5, 0), (5, 5), (2 ** 31, 1)):
        assert h.dyk_tensor_stats_ws_bytes(items, nbuf) == 0
    refused = [dict(nbuf=0), dict(nbuf=5), dict(nseg=0), dict(nseg=-1), dict(nitems=2), dict(buf0=None), dict(buf1=None),
               dict(buf1=0x1008), dict(seg=None), dict(seg=0x10004), dict(items=None), dict(items=0x20004), dict(ws=None),
               dict(ws=0x30004), dict(out=None), dict(out=0x40004), dict(ws_bytes=239), dict(ws_bytes=0), dict(n=0), dict(n=4098),
               dict(n=-4)]
    for kw in refused:
        assert h.dyk_tensor_stats(ctypes.byref(_desc(lib, **kw)), None) == -1, kw
