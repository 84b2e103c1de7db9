"""Row-wise multi-label NMS on the GPU (dyk_nms_rows; the multi_label branch of reference build_utils/utils.py:422-424).

Yardsticks: oracle.nms.non_max_suppression(..., return_indices=True) on the CPU and dyk_nms_ex on the same device tensor.
Everything is compared exactly: values as bit patterns (uint32 views), rows and counts as integers.  Every direct call gets
its workspace with 0xA5 frames in front of and behind exactly dyk_nms_rows_workspace_bytes bytes of every image, and `out`,
`out_rows`, `counts`, `n_cand` pre-filled with sentinels: the frames must be intact and `out` / `out_rows` beyond `count`
must still hold the sentinel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nms_rows_cases as RC

pytestmark = pytest.mark.gpu

SENT_F, SENT_I, FRAME = -12345.5, -77, 512


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _dev(name):
    return RC.pred(name).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _oracle(name, agnostic=False, classes=None, max_num=RC.MAX_NUM):
    from oracle import nms as onms
    return onms.non_max_suppression(RC.pred(name), conf_thres=RC.MATRIX[name]["conf"], iou_thres=RC.IOU, multi_label=True,
                                    classes=list(classes) if classes else None, agnostic=agnostic, max_num=max_num,
                                    return_indices=True)


def _run(pred, entry, flags, conf, iou=RC.IOU, agnostic=False, classes=None, max_num=RC.MAX_NUM, cand_cap=None):
    """one launch of dyk_nms_rows ("rows") or dyk_nms_ex ("ex", multi_label = 1) -> dict of host arrays"""
    from dyk import lib as L
    h = L.load()
    B, N, no = pred.shape
    out = torch.full((B, max_num, 6), SENT_F, device="cuda")
    rows = torch.full((B, max_num), SENT_I, dtype=torch.int32, device="cuda")
    counts = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    n_cand = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    if entry == "rows":
        per = int(h.dyk_nms_rows_workspace_bytes(N, cand_cap))
        stride = per + FRAME
        buf = torch.full((FRAME + B * stride,), 0xA5, dtype=torch.uint8, device="cuda")
        d = L.DykNmsRowsDesc()
        d.ws, d.ws_per_image = buf.data_ptr() + FRAME, stride
        d.cand_cap, d.n_cand = cand_cap, n_cand.data_ptr()
    else:
        per = int(h.dyk_nms_workspace_bytes(N, no, 1))
        buf = torch.empty(B * per, dtype=torch.uint8, device="cuda")
        d = L.DykNmsDesc()
        d.ws, d.ws_per_image = buf.data_ptr(), per
    d.pred, d.out, d.out_rows, d.counts = pred.data_ptr(), out.data_ptr(), rows.data_ptr(), counts.data_ptr()
    d.B, d.N, d.no, d.conf_thres, d.iou_thres = B, N, no, conf, iou
    d.multi_label, d.agnostic, d.max_num = 1, 1 if agnostic else 0, max_num
    cl = list(classes) if classes else []
    d.n_classes = len(cl)
    for i, c in enumerate(cl):
        d.classes[i] = c
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = h.dyk_nms_rows(ctypes.byref(d), flags, s) if entry == "rows" else h.dyk_nms_ex(ctypes.byref(d), flags, s)
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    r = dict(out=out.cpu().numpy(), rows=rows.cpu().numpy(), counts=counts.cpu().numpy(), n_cand=n_cand.cpu().numpy())
    if entry == "rows":
        w = buf.cpu().numpy()
        frames = [w[:FRAME]] + [w[FRAME + b * stride + per:FRAME + (b + 1) * stride] for b in range(B)]
        r["frames_ok"] = all(bool((f == 0xA5).all()) for f in frames)
        cand_bytes = per - (8 * N + 255) // 256 * 256                 # keys + candidates, in front of the per-row arrays
        r["cand_area_untouched"] = [bool((w[FRAME + b * stride:FRAME + b * stride + cand_bytes] == 0xA5).all()) for b in range(B)]
    return r


def _check_sentinels(r, what):
    assert r["frames_ok"], what
    for b, n in enumerate(r["counts"]):
        k = max(int(n), 0)
        assert (r["out"][b, k:] == np.float32(SENT_F)).all() and (r["rows"][b, k:] == SENT_I).all(), (what, b)
        if n < 0:
            assert r["cand_area_untouched"][b], (what, b)


def _same_as_ex(r, e, what):
    assert np.array_equal(r["counts"], e["counts"]), (what, r["counts"], e["counts"])
    assert np.array_equal(_bits(r["out"]), _bits(e["out"])), what         # whole arrays: the sentinel tails too
    assert np.array_equal(r["rows"], e["rows"]), what


def _same_as_oracle(r, want, want_rows, what, images=None):
    for b in (range(len(want)) if images is None else images):
        n = int(r["counts"][b])
        if want[b] is None:
            assert n == 0, (what, b, n)
            continue
        assert n == want[b].shape[0], (what, b, n, want[b].shape)
        assert np.array_equal(_bits(r["out"][b, :n]), _bits(want[b].numpy())), (what, b)
        assert np.array_equal(r["rows"][b, :n], want_rows[b].numpy().astype(np.int32)), (what, b)


VARIANTS = [(name, False, None, RC.MAX_NUM) for name in RC.MATRIX]
VARIANTS += [("s33", True, None, RC.MAX_NUM), ("ties3", True, None, RC.MAX_NUM)]
VARIANTS += [("s80", False, tuple(RC.S80_CLASSES), RC.MAX_NUM)]
VARIANTS += [("s20", False, None, 1), ("s20", False, None, 512)]


def _vid(v):
    name, agnostic, classes, max_num = v
    return name + ("-agnostic" if agnostic else "") + ("-classes16" if classes else "") + ("-max%d" % max_num if max_num != RC.MAX_NUM else "")


@pytest.mark.parametrize("merge", [0, 1], ids=["plain", "merge"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_matrix_through_the_direct_entry(variant, merge):
    from dyk import detect
    name, agnostic, classes, max_num = variant
    conf = RC.MATRIX[name]["conf"]
    _, want_n = RC.candidate_counts(RC.pred(name), conf, classes)
    cap = max(detect.nms_default_candidates(RC.MATRIX[name]["N"]), max(want_n))      # fits
    kw = dict(conf=conf, agnostic=agnostic, classes=classes, max_num=max_num)
    r = _run(_dev(name), "rows", merge, cand_cap=cap, **kw)
    e = _run(_dev(name), "ex", merge, **kw)
    what = (_vid(variant), merge)
    assert r["n_cand"].tolist() == want_n, what
    assert (r["counts"] > 0).all(), what
    _check_sentinels(r, what)
    _same_as_ex(r, e, what)
    if not merge:
        want, want_rows = _oracle(name, agnostic, classes, max_num)
        _same_as_oracle(r, want, want_rows, what)
    if name == "s20" and max_num in (1, 512):
        assert (r["counts"] == 1).all() if max_num == 1 else (r["counts"] > 1).all()


@pytest.mark.parametrize("nc", RC.EDGE_NC)
@pytest.mark.parametrize("N", RC.EDGE_N)
def test_wave_and_chunk_edges(N, nc):
    """dense rows: every row alive, about half of the classes passing; N around one wavefront and one 1024-row turn, nc around
    one and two 64-class chunks"""
    p = RC.dense_pred(2, N, nc, 1000 * N + nc)
    alive, want_n = RC.candidate_counts(p, RC.DENSE_CONF)
    assert alive == [N, N]
    if N * nc >= 4000:                                                    # (binomial(N * nc, 0.5): 0.4 .. 0.6 is > 12 sigma wide)
        assert all(0.4 * N * nc < k < 0.6 * N * nc for k in want_n)
    dev = p.cuda()
    for merge in (0, 1):
        r = _run(dev, "rows", merge, conf=RC.DENSE_CONF, cand_cap=max(max(want_n), 1))   # the capacity is exactly the largest count
        e = _run(dev, "ex", merge, conf=RC.DENSE_CONF)
        assert r["n_cand"].tolist() == want_n, (N, nc, merge)
        _check_sentinels(r, (N, nc, merge))
        _same_as_ex(r, e, (N, nc, merge))
        if not merge and (N, nc) in RC.EDGE_ORACLE:
            from oracle import nms as onms
            want, want_rows = onms.non_max_suppression(p, conf_thres=RC.DENSE_CONF, iou_thres=RC.IOU, multi_label=True,
                                                       return_indices=True)
            _same_as_oracle(r, want, want_rows, (N, nc))


@pytest.mark.parametrize("nc", [3, 4, 5, 16, 17, 32, 33])
@pytest.mark.parametrize("N", [65, 1025])
def test_rows_that_share_a_wavefront(N, nc):
    """up to 32 classes a row takes the power of two >= nc lanes and a wavefront holds several rows side by side: class counts
    at, below and above each width, row counts that leave the last wavefront partly filled"""
    p = RC.dense_pred(2, N, nc, 2000 * N + nc)
    alive, want_n = RC.candidate_counts(p, RC.DENSE_CONF)
    assert alive == [N, N] and min(want_n) > 0
    dev = p.cuda()
    for merge in (0, 1):
        r = _run(dev, "rows", merge, conf=RC.DENSE_CONF, cand_cap=max(want_n))
        e = _run(dev, "ex", merge, conf=RC.DENSE_CONF)
        assert r["n_cand"].tolist() == want_n, (N, nc, merge)
        _check_sentinels(r, (N, nc, merge))
        _same_as_ex(r, e, (N, nc, merge))


def test_special_values():
    """NaN, +inf, -0.0 in obj, in one class score, in w and h; obj and conf equal to conf_thres; w, h equal to 2 and 4096; a middle
    image without an alive row; an image whose alive rows have no passing class"""
    p, what = RC.special_pred()
    alive, want_n = RC.candidate_counts(p, RC.SPECIAL_CONF)
    assert alive[1] == 0 and alive[2] == 96 and want_n[1:] == [0, 0] and want_n[0] > 0
    dev = p.cuda()
    for merge in (0, 1):
        r = _run(dev, "rows", merge, conf=RC.SPECIAL_CONF, cand_cap=8192)
        e = _run(dev, "ex", merge, conf=RC.SPECIAL_CONF)
        assert r["n_cand"].tolist() == want_n
        assert r["counts"][1] == 0 and r["counts"][2] == 0 and r["counts"][0] > 0
        _check_sentinels(r, merge)
        _same_as_ex(r, e, merge)
        if not merge:
            kept = set(r["rows"][0, :r["counts"][0]].tolist())
            gone = [k for k in what if k not in ("obj_inf", "cls_inf", "cls_nan", "cls_neg0")]
            assert not kept & {what[k] for k in gone}, sorted(k for k in gone if what[k] in kept)
            assert what["obj_inf"] in kept                                # inf * cls = inf > conf_thres: a candidate, scored first
            assert np.isinf(r["out"][0, 0, 4])


def test_capacity_below_the_count_marks_the_image_and_writes_nothing():
    name, cap = "s80_cap", 2100
    conf = RC.MATRIX[name]["conf"]
    _, want_n = RC.candidate_counts(RC.pred(name), conf)
    assert want_n[0] <= cap < min(want_n[1:])
    want, want_rows = _oracle(name)
    for merge in (0, 1):
        r = _run(_dev(name), "rows", merge, conf=conf, cand_cap=cap)
        e = _run(_dev(name), "ex", merge, conf=conf)
        assert r["n_cand"].tolist() == want_n                             # exact also where the image overflows
        assert r["counts"][1] == -1 and r["counts"][2] == -1 and r["counts"][0] == e["counts"][0] > 0
        _check_sentinels(r, merge)                                        # images 1, 2: out, out_rows, keys, candidates untouched
        assert np.array_equal(_bits(r["out"][0]), _bits(e["out"][0])) and np.array_equal(r["rows"][0], e["rows"][0])
        if not merge:
            _same_as_oracle(r, want, want_rows, "capacity 2100", images=[0])
        full = _run(_dev(name), "rows", merge, conf=conf, cand_cap=max(want_n))   # exactly the largest count: all complete
        assert full["n_cand"].tolist() == want_n and (full["counts"] > 0).all()
        _check_sentinels(full, merge)
        _same_as_ex(full, e, merge)
        if not merge:
            _same_as_oracle(full, want, want_rows, "capacity = largest count")


def _wrapper_equals_oracle(name, **kw):
    from build_utils.utils import non_max_suppression as api
    from dyk import detect
    want, want_rows = _oracle(name)
    conf = RC.MATRIX[name]["conf"]
    got, rows = detect.non_max_suppression(_dev(name), conf_thres=conf, iou_thres=RC.IOU, multi_label=True, return_rows=True, **kw)
    pub = api(_dev(name), conf_thres=conf, iou_thres=RC.IOU, **kw)
    for b in range(RC.B):
        assert np.array_equal(_bits(got[b].cpu().numpy()), _bits(want[b].numpy())), (name, b)
        assert np.array_equal(_bits(pub[b].cpu().numpy()), _bits(want[b].numpy())), (name, b)
        assert rows[b].cpu().tolist() == want_rows[b].tolist(), (name, b)


def test_wrapper_runs_an_overflowing_batch_again_on_the_per_image_route():
    from dyk import detect
    c0 = detect.nms_route_counts()
    _wrapper_equals_oracle("s80_cap", candidates=2100)                    # two calls: dyk.detect and build_utils.utils
    c1 = detect.nms_route_counts()
    assert c1["rows_overflow"] - c0["rows_overflow"] == 2 and c1["rows"] - c0["rows"] == 2 and c1["image"] - c0["image"] == 2
    from build_utils.utils import non_max_suppression as api
    api(_dev("s80_cap"), conf_thres=RC.MATRIX["s80_cap"]["conf"], iou_thres=RC.IOU, candidates=2100)
    assert detect.nms_route_counts()["rows_overflow"] - c1["rows_overflow"] == 1      # one call, one overflow
    _wrapper_equals_oracle("s80_cap", candidates=2318)                    # the largest count fits: no second launch
    c2 = detect.nms_route_counts()
    assert c2["rows_overflow"] == c1["rows_overflow"] + 1 and c2["image"] == c1["image"] + 1


def test_wrapper_with_the_default_capacity_on_365_classes():
    from dyk import detect
    _, n = RC.candidate_counts(RC.pred("s365"), RC.MATRIX["s365"]["conf"])
    assert min(n) > detect.nms_default_candidates(700) == 8192
    c0 = detect.nms_route_counts()
    _wrapper_equals_oracle("s365")
    c1 = detect.nms_route_counts()
    assert c1["rows_overflow"] - c0["rows_overflow"] == 2 and c1["image"] - c0["image"] == 2


def test_best_class_and_one_class_calls_keep_the_per_image_route():
    from dyk import detect
    c0 = detect.nms_route_counts()
    detect.non_max_suppression(_dev("s20"), conf_thres=0.5, multi_label=False)
    detect.non_max_suppression(_dev("s20")[..., :6].contiguous(), conf_thres=0.5, multi_label=True)
    c1 = detect.nms_route_counts()
    assert c1["image"] - c0["image"] == 2 and c1["rows"] == c0["rows"] and c1["rows_overflow"] == c0["rows_overflow"]


def test_peak_memory_of_a_multi_label_call_at_80_classes():
    """[4, 3000, 85]: the per-pair workspace is 4 * dyk_nms_workspace_bytes(3000, 85, 1) = 35.3 MB; the call may raise the
    peak allocation by less than a quarter of that"""
    import sys
    from helpers import GOLDEN
    sys.path.insert(0, GOLDEN)
    import cases
    from dyk import detect, lib as L
    p = cases.nms_pred(dict(name="mem", B=4, N=3000, nc=80, kind="sparse", seed=78))
    _, n = RC.candidate_counts(p, 0.6)
    assert 0 < max(n) <= detect.nms_default_candidates(3000)              # no image overflows
    dev = p.cuda().contiguous()
    full = 4 * int(L.load().dyk_nms_workspace_bytes(3000, 85, 1))
    c0 = detect.nms_route_counts()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = detect.non_max_suppression(dev, conf_thres=0.6, iou_thres=RC.IOU, multi_label=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    c1 = detect.nms_route_counts()
    print("peak allocation rises by %d bytes; per-pair workspace %d bytes (x %.1f)" % (rise, full, full / max(rise, 1)))
    assert c1["rows"] == c0["rows"] + 1 and c1["rows_overflow"] == c0["rows_overflow"] and c1["image"] == c0["image"]
    assert all(g is not None for g in got)
    assert rise < full / 4


def test_two_runs_are_bit_identical():
    conf = RC.MATRIX["s80"]["conf"]
    a = _run(_dev("s80"), "rows", 1, conf=conf, cand_cap=8192)
    junk = torch.full((1 << 20,), float("nan"), device="cuda")            # the second run's buffers start from other bits
    del junk
    b = _run(_dev("s80"), "rows", 1, conf=conf, cand_cap=8192)
    assert np.array_equal(_bits(a["out"]), _bits(b["out"])) and np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["n_cand"], b["n_cand"])
    assert (a["counts"] > 0).all()
