"""Multi-class evaluator on the GPU (dyk_eval_match, dyk.evalmap.DetectionEvaluator) against tests/map_ref.py.

Everything is compared exactly -- integers, or IEEE operations in a fixed order: tp_mask, match, cls, the bits of conf, the
bits of the scaled box (against scale_coords + clip_coords of build_utils.utils on the same rows) and the bits of the fp64
IoU.  Shapes and rules: tests/map_cases.py (0 / 1 / 63 / 64 / 65 / 1024 boxes per image, max_num 8 and 100, nc 1 / 3 / 80,
1 / 10 / 16 thresholds, an image without detections; the hand-built cases pin one matching rule each)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import map_cases as MC
import map_ref

pytestmark = pytest.mark.gpu


def _case(name):
    return MC.HAND[name] if name in MC.HAND else MC.case(name)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _sub_targets(labels):
    t = MC.targets_of(labels)
    return torch.from_numpy(t).cuda() if t.shape[0] else torch.zeros((0, 6), device="cuda")


@functools.lru_cache(maxsize=None)
def _inputs(name, letterbox):
    """(detections as the evaluator gets them, per-image ratio_pad or None, detections in the original frame for map_ref).
    Letterboxed: the original-frame boxes are what scale_coords + clip_coords make of the same rows on the device."""
    from build_utils.utils import clip_coords, scale_coords
    c = _case(name)
    if not letterbox:
        return c["dets"], None, c["dets"]
    raw, rps = MC.letterboxed(c)
    back = []
    for d, rp, (w, h) in zip(raw, rps, c["shapes"]):
        if d is None:
            back.append(None)
            continue
        t = torch.from_numpy(d).cuda()
        boxes = scale_coords(MC.IMG1, t[:, :4].clone(), (h, w), rp)
        clip_coords(boxes, (h, w))
        back.append(np.concatenate([boxes.cpu().numpy(), d[:, 4:]], 1))
    return raw, rps, back


@functools.lru_cache(maxsize=None)
def _ref(name, letterbox=False):
    c = _case(name)
    return map_ref.evaluate(_inputs(name, letterbox)[2], c["labels"], c["shapes"], c["nc"], c["thresholds"])


def _evaluate(name, letterbox=False, form="padded", splits=None, fill=0.0):
    from dyk.evalmap import DetectionEvaluator
    c = _case(name)
    dets, rps, _ = _inputs(name, letterbox)
    ev = DetectionEvaluator(c["nc"], c["thresholds"])
    B = len(dets)
    for lo, hi in splits or [(0, B)]:
        out, counts = MC.padded_of(dets[lo:hi], c["max_num"], fill)
        out = torch.from_numpy(out).cuda()
        arg = (out, counts) if form == "padded" else [out[b, :n] if n else None for b, n in enumerate(counts)]
        if form == "copies":                            # a list that is NOT a set of views of one padded tensor
            arg = [None if d is None else d.clone() for d in arg]
        ev.update(arg, _sub_targets(c["labels"][lo:hi]), c["shapes"][lo:hi], img1_shape=MC.IMG1 if letterbox else None,
                  ratio_pad=rps[lo:hi] if letterbox else None)
    return ev


def _assert_records(got, want):
    assert got["conf"].shape == want["conf"].shape
    for k in ("tp_mask", "match", "cls"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k])[0][:8])
    for k in ("conf", "box", "iou"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.nonzero(_bits(got[k]) != _bits(want[k]))[0][:8])


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("name", sorted(MC.MATRIX))
def test_records_equal_the_reference_field_by_field(name, letterbox):
    ev = _evaluate(name, letterbox)
    r = _ref(name, letterbox)
    _assert_records(ev.records(), r["records"])
    res = ev.compute()
    assert np.array_equal(res["ap"], r["ap"], equal_nan=True) and np.array_equal(res["lamr"], r["lamr"], equal_nan=True)
    assert np.array_equal(ev.n_gt, r["n_gt"]) and ev.num_imgs == 5


@pytest.mark.parametrize("name", sorted(MC.HAND))
def test_hand_built_rules(name):
    rec = _evaluate(name).records()
    _assert_records(rec, _ref(name)["records"])
    if name == "exact_half":            # 100 / 200 is a TP at 0.5, 90 / 200 is not
        assert rec["iou"][0] == 0.5 and rec["tp_mask"].tolist() == [1, 0]
    if name == "twins":                 # the first of two identical boxes wins; the second is never a second choice
        assert rec["match"].tolist() == [0, 0] and rec["tp_mask"].tolist() == [1, 0]
    if name == "other_class":           # a detection whose class has no box in the image
        assert rec["match"].tolist() == [-1, 0, -1] and rec["iou"].tolist() == [0.0, 1.0, 0.0] and rec["tp_mask"].tolist() == [0, 1, 0]
    if name == "per_threshold":
        assert rec["tp_mask"].tolist() == [1, 2]
    if name == "hand_map":
        res = _evaluate(name).compute()
        assert res["map50"] == pytest.approx(5 / 12, abs=1e-15) and np.isnan(res["ap"][2, 0])


@pytest.mark.parametrize("name", ["nc3_t10_m100", "nc80_t16_m100"])
def test_three_updates_equal_one(name):
    one, three = _evaluate(name, True), _evaluate(name, True, splits=[(0, 2), (2, 3), (3, 5)])
    a, b = one.records(), three.records()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    ra, rb = one.compute(), three.compute()
    assert np.array_equal(ra["ap"], rb["ap"], equal_nan=True) and np.array_equal(ra["lamr"], rb["lamr"], equal_nan=True)
    assert ra["map"] == rb["map"]


def test_the_same_run_twice_gives_the_same_bytes_in_every_input_form():
    runs = [_evaluate("nc80_t16_m100", True, form=f).records() for f in ("padded", "padded", "list", "copies")]
    for other in runs[1:]:
        for k in runs[0]:
            assert runs[0][k].tobytes() == other[k].tobytes(), k


def test_records_grow_past_the_first_capacity():
    from dyk.evalmap import DetectionEvaluator
    c = _case("nc3_t10_m100")
    ev = DetectionEvaluator(c["nc"], c["thresholds"])
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    out, tg = torch.from_numpy(out).cuda(), _sub_targets(c["labels"])
    reps = 1024 // sum(counts) + 2
    for _ in range(reps):
        ev.update((out, counts), tg, c["shapes"])
    rec, want = ev.records(), _ref("nc3_t10_m100")["records"]
    n = sum(counts)
    assert rec["conf"].shape[0] == reps * n > 1024
    for i in (0, reps - 1):
        assert np.array_equal(rec["tp_mask"][i * n:(i + 1) * n], want["tp_mask"])
        m = want["match"].copy()
        m[m >= 0] += i * tg.shape[0]
        assert np.array_equal(rec["match"][i * n:(i + 1) * n], m)


SENT_F, SENT_I = -12345.5, -77


def _direct(c, rec_off, cap, T=None, nc=None, counts=None):
    """one direct launch into sentinel-filled arrays -> (return code, host arrays, error words)"""
    from dyk import lib as L
    out, cnt = MC.padded_of(c["dets"], c["max_num"], SENT_F)
    cnt = cnt if counts is None else counts
    B = len(cnt)
    keep = {"out": torch.from_numpy(out).cuda(), "counts": torch.tensor(cnt, dtype=torch.int32).cuda(),
            "rec_off": torch.tensor(rec_off, dtype=torch.int32).cuda(), "targets": _sub_targets(c["labels"]),
            "gt_off": torch.tensor(np.concatenate(([0], np.cumsum([l.shape[0] for l in c["labels"]]))), dtype=torch.int32).cuda(),
            "shape0": torch.tensor(c["shapes"], dtype=torch.int32).cuda(), "err": torch.zeros(2, dtype=torch.int32).cuda(),
            "conf": torch.full((cap,), SENT_F).cuda(), "cls": torch.full((cap,), SENT_I, dtype=torch.int32).cuda(),
            "tp_mask": torch.full((cap,), SENT_I, dtype=torch.int32).cuda(), "match": torch.full((cap,), SENT_I, dtype=torch.int32).cuda(),
            "iou": torch.full((cap,), SENT_F, dtype=torch.float64).cuda(), "box": torch.full((cap, 4), SENT_F).cuda()}
    d = L.DykEvalMatchDesc()
    for k, v in keep.items():
        setattr(d, k, v.data_ptr())
    d.unpad = None
    thr = c["thresholds"]
    for t, v in enumerate(thr):
        d.thr[t] = v
    d.B, d.max_num, d.nt, d.nc, d.T, d.rec_cap = B, c["max_num"], keep["targets"].shape[0], c["nc"] if nc is None else nc, len(thr) if T is None else T, cap
    rc = L.load().dyk_eval_match(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: keep[k].cpu().numpy() for k in ("conf", "cls", "tp_mask", "match", "iou", "box")}, keep["err"].cpu().tolist()


@pytest.mark.parametrize("name", ["nc3_t16_m8_full", "nc80_t16_m100"])
def test_nothing_is_written_outside_an_images_records(name):
    """records with gaps between the images, sentinel-framed: only [rec_off[b], rec_off[b] + counts[b]) changes, and holds
    what the reference says; an image with counts -1 (an overflowed dyk_nms_rows image) writes nothing"""
    c = _case(name)
    counts = [0 if d is None else d.shape[0] for d in c["dets"]]
    gap = 5
    rec_off = [7 + b * (c["max_num"] + gap) for b in range(5)]
    cap = rec_off[-1] + c["max_num"] + 9
    rc, got, err = _direct(c, rec_off, cap)
    assert rc == 0 and err == [0, 0]
    want = _ref(name)["records"]
    written = np.zeros(cap, dtype=bool)
    first = 0
    for b, n in enumerate(counts):
        s, w = slice(rec_off[b], rec_off[b] + n), slice(first, first + n)
        written[s] = True
        assert np.array_equal(got["tp_mask"][s].view(np.uint32), want["tp_mask"][w]) and np.array_equal(got["match"][s], want["match"][w])
        assert np.array_equal(_bits(got["iou"][s]), _bits(want["iou"][w])) and np.array_equal(_bits(got["box"][s]), _bits(want["box"][w]))
        assert np.array_equal(got["cls"][s], want["cls"][w]) and np.array_equal(_bits(got["conf"][s]), _bits(want["conf"][w]))
        first += n
    for k in ("cls", "tp_mask", "match"):
        assert (got[k][~written] == SENT_I).all(), k
    for k in ("conf", "iou", "box"):
        assert (got[k][~written] == SENT_F).all(), k
    minus = [-1 if b == 0 else n for b, n in enumerate(counts)]
    rc, got, err = _direct(c, rec_off, cap, counts=minus)
    assert rc == 0 and (got["cls"][:rec_off[1]] == SENT_I).all() and (got["conf"][:rec_off[1]] == SENT_F).all()


def test_the_kernel_refuses_tables_that_leave_the_arrays():
    """records past rec_cap: the image writes nothing and the second error word is set (no out-of-bounds store)"""
    c = _case("nc1_t1_m8")
    counts = [0 if d is None else d.shape[0] for d in c["dets"]]
    rec_off = [0, 8, 16, 24, 32]
    assert counts[4] > 1
    rc, got, err = _direct(c, rec_off, cap=rec_off[4] + counts[4] - 1)        # the last record of image 4 does not fit
    assert rc == 0 and err == [0, 1]
    assert (got["cls"][rec_off[4]:] == SENT_I).all() and (got["cls"][rec_off[2]:rec_off[2] + counts[2]] != SENT_I).all()
    from dyk import lib as L
    assert _direct(c, rec_off, 64, T=17)[0] == -1 and _direct(c, rec_off, 64, T=0)[0] == -1
    assert L.load().dyk_eval_match(None, None) == -1


def _pred(nc, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = 3, 300
    p = torch.rand(B, N, 5 + nc, generator=g)
    p[..., :2] = p[..., :2] * 200 + 20
    p[..., 2:4] = p[..., 2:4] * 40 + 8
    p[..., 4] = p[..., 4] ** 3
    p[2, :, 4] = 0.0                                    # an image without detections
    return p.cuda()


@pytest.mark.parametrize("nc,multi,route", [(1, False, "image"), (3, True, "rows")])
def test_return_padded_gives_the_same_tensors_as_the_list(nc, multi, route):
    from build_utils.utils import non_max_suppression
    from dyk import detect
    p = _pred(nc, 11 + nc)
    before = detect.nms_route_counts()
    lst = non_max_suppression(p, conf_thres=0.3, iou_thres=0.6, multi_label=multi)
    out, counts = non_max_suppression(p, conf_thres=0.3, iou_thres=0.6, multi_label=multi, return_padded=True)
    after = detect.nms_route_counts()
    assert after[route] - before[route] == 2 and sum(after.values()) - sum(before.values()) == 2
    assert out.shape == (3, 100, 6) and len(counts) == 3 and counts[2] == 0 and max(counts) > 0
    for b, d in enumerate(lst):
        assert (d is None) == (counts[b] == 0)
        if d is not None:
            assert d.shape[0] == counts[b] and torch.equal(d, out[b, :counts[b]])


def test_refusals():
    from dyk import lib as L
    from dyk.evalmap import DetectionEvaluator
    with pytest.raises(ValueError, match="17"):
        DetectionEvaluator(1, [0.1 + 0.05 * i for i in range(17)])
    c = _case("nc3_t10_m100")
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    out, tg = torch.from_numpy(out).cuda(), _sub_targets(c["labels"])
    ev = DetectionEvaluator(3, (0.5,))
    with pytest.raises(L.DykError):
        ev.update((out.cpu(), counts), tg, c["shapes"])
    with pytest.raises(L.DykError):
        ev.update((out, counts), tg.cpu(), c["shapes"])
    crowded = torch.zeros((1025, 6), device="cuda")
    crowded[:, 0] = 3
    crowded[:, 2:] = 0.1
    with pytest.raises(ValueError, match="image 3 .*1025"):
        ev.update((out, counts), crowded, c["shapes"])
    assert ev.num_imgs == 0 and ev.n_gt.sum() == 0 and ev.records()["conf"].shape[0] == 0        # a refused batch leaves no trace
    ev = DetectionEvaluator(2, (0.5,))                   # the case's detections carry class 2
    ev.update((out, counts), torch.zeros((0, 6), device="cuda"), c["shapes"])
    with pytest.raises(ValueError, match="class"):
        ev.compute()
    bad = ev.records()
    assert (bad["tp_mask"] == 0).all() and (bad["match"] == -1).all() and (bad["iou"] == 0).all()
    ev.reset()
    assert ev.compute()["ap"].shape == (2, 1)


def test_the_64_pair_fixture_end_to_end(tiles):
    """the detections of the 64-pair fixture (tests/test_eval_ap.py: _state5 / _ap5, fp32) through the evaluator with one class:
    AP and LAMR EQUAL to what compute_ap_lamr makes of the same detections, one record per detection"""
    import test_eval_ap as TE
    from build_utils.parse_config import materialize_cfg
    from build_utils.utils import non_max_suppression, scale_coords
    from dyk.evalmap import DetectionEvaluator
    from models import YOLO
    from other_utils.metrics import compute_ap_lamr
    R5 = TE.R5
    _, sd = TE._state5()
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(R5.CFG))
    m.load_state_dict(sd)
    m.dyk_dtype = "fp32"
    m = m.cuda().eval()
    v, l, targets = R5.dataset()
    with torch.no_grad():
        io = torch.cat([m(v[c:c + 16].cuda().float() / 255.0, l[c:c + 16].cuda().float() / 255.0)[0].clone() for c in range(0, 64, 16)])
    dets = non_max_suppression(io, conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
    want, ndet = TE._ap5(dets, scale_coords, compute_ap_lamr, targets)
    shapes = [(R5.SHAPE0[1], R5.SHAPE0[0])] * 64
    ev = DetectionEvaluator(1, (0.5,))
    ev.update(dets, targets.cuda(), shapes, img1_shape=(R5.H, R5.W), ratio_pad=R5.RATIO_PAD)
    res = ev.compute()
    print("64-pair fixture: AP %.5f LAMR %.5f from %d records (compute_ap_lamr: %.5f / %.5f)"
          % (res["ap"][0, 0], res["lamr"][0, 0], ev.records()["conf"].shape[0], want["ap"], want["lamr"]))
    assert res["ap"][0, 0] == want["ap"] and res["lamr"][0, 0] == want["lamr"] and res["map50"] == want["ap"]
    assert np.array_equal(res["recall"][0][0], want["recall"]) and np.array_equal(res["precision"][0][0], want["precision"])
    assert ev.records()["conf"].shape[0] == ndet == int(TE.GOLD5["ndet"].sum()) == 910
    # and batch by batch, as an evaluation loop feeds it
    ev.reset()
    for c in range(0, 64, 16):
        tb = targets[(targets[:, 0] >= c) & (targets[:, 0] < c + 16)].clone()
        tb[:, 0] -= c
        ev.update(dets[c:c + 16], tb.cuda(), shapes[c:c + 16], img1_shape=(R5.H, R5.W), ratio_pad=R5.RATIO_PAD)
    again = ev.compute()
    assert again["ap"][0, 0] == want["ap"] and again["lamr"][0, 0] == want["lamr"]
