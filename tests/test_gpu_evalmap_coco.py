"""COCO-protocol evaluator on the GPU (dyk_eval_match_coco, dyk.evalmap.CocoEvaluator) against tests/coco_ref.py.

Every record field is compared exactly -- integers, or IEEE operations in a fixed order: dtm, dtig, match, rank, img, cls,
the bits of conf, of the box as used (against scale_coords + clip_coords of build_utils.utils on the same rows, then rint)
and of the fp64 detection area.  precision / recall exactly, the stats within 1e-10 (tests/test_coco_reference.py says why).
Shapes and rules: tests/coco_cases.py.  Nothing here is pinned against pycocotools: there is none to run."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import coco_cases as CC
import coco_ref
import map_cases as MC

pytestmark = pytest.mark.gpu

CUSTOM = {
    "thr16_area1": lambda: CC.custom("nc3_m100", [round(0.2 + 0.05 * i, 2) for i in range(15)] + [1.0], [(0.0, 1e10)]),
    "thr4_area4": lambda: CC.custom("nc1_m160", (0.5, 0.75, 0.3, 0.95), [(0.0, 1e10), (0.0, 400.0), (400.0, 400.0 * 16), (2000.0, 1e5)]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    if name in CUSTOM:
        return CUSTOM[name]()
    return CC.HAND[name] if name in CC.HAND else CC.case(name)


def _params(c):
    return c.get("thresholds", coco_ref.THRESHOLDS), c.get("areas", coco_ref.AREAS), c.get("max_dets", coco_ref.MAX_DETS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _sub_targets(labels):
    t = MC.targets_of(labels)
    return torch.from_numpy(t).cuda() if t.shape[0] else torch.zeros((0, 6), device="cuda")


@functools.lru_cache(maxsize=None)
def _inputs(name, letterbox):
    """(detections as the evaluator gets them, per-image ratio_pad or None, detections in the original frame for coco_ref).
    Letterboxed: the original-frame boxes are what scale_coords + clip_coords make of the same rows on the device."""
    from build_utils.utils import clip_coords, scale_coords
    c = _case(name)
    if not letterbox:
        return c["dets"], None, c["dets"]
    raw, rps = MC.letterboxed({"dets": c["dets"], "shapes": c["shapes"]})
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
def _ref(name, letterbox=False, round_boxes=True):
    c = _case(name)
    return coco_ref.evaluate(_inputs(name, letterbox)[2], c["labels"], c["shapes"], c["nc"], *_params(c), round_boxes=round_boxes)


def _evaluate(name, letterbox=False, round_boxes=True, form="padded", splits=None, fill=0.0):
    from dyk.evalmap import CocoEvaluator
    c = _case(name)
    dets, rps, _ = _inputs(name, letterbox)
    thr, areas, max_dets = _params(c)
    ev = CocoEvaluator(c["nc"], thr, areas, max_dets, round_boxes=round_boxes)
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


INT_FIELDS, FLOAT_FIELDS = ("cls", "img", "rank", "dtm", "dtig"), ("conf", "box", "darea")


def _assert_records(got, ref):
    want = dict(ref["records"], match=ref["match_global"])
    assert got["conf"].shape == want["conf"].shape and got["match"].shape == want["match"].shape
    for k in INT_FIELDS + ("match",):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:8].tolist())
    for k in FLOAT_FIELDS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:8].tolist())


def _assert_result(res, ref):
    assert np.array_equal(res["precision"], ref["precision"]) and np.array_equal(res["recall"], ref["recall"])
    assert np.abs(np.array(res["stats"]) - np.array(ref["stats"])).max() <= 1e-10


@pytest.mark.parametrize("round_boxes", [True, False])
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("name", sorted(CC.MATRIX))
def test_records_equal_the_reference_field_by_field(name, letterbox, round_boxes):
    ev = _evaluate(name, letterbox, round_boxes)
    r = _ref(name, letterbox, round_boxes)
    _assert_records(ev.records(), r)
    _assert_result(ev.compute(), r)
    assert np.array_equal(ev.n_gt_ka, r["npig"]) and ev.num_imgs == 5


@pytest.mark.parametrize("round_boxes", [True, False])
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("name", sorted(CC.HAND))
def test_hand_built_rules(name, letterbox, round_boxes):
    ev = _evaluate(name, letterbox, round_boxes)
    r = _ref(name, letterbox, round_boxes)
    rec, res = ev.records(), ev.compute()
    _assert_records(rec, r)
    _assert_result(res, r)
    if not letterbox:                   # the written answers hold for the exact coordinates (one image each, or local rows)
        first = np.concatenate(([0], np.cumsum([lab.shape[0] for lab in _case(name)["labels"]])))[rec["img"]]
        local = dict(rec, match=np.where(rec["match"] >= 0, rec["match"] - first[:, None, None], -1))
        CC.check_hand(name, local, res["stats"], ev.n_gt_ka, round_boxes)


@pytest.mark.parametrize("name", sorted(CUSTOM))
def test_custom_thresholds_and_area_ranges(name):
    """16 thresholds (the last one 1.0) with one area range; 4 unsorted thresholds with 4 ranges of other bounds"""
    for letterbox in (False, True):
        ev = _evaluate(name, letterbox)
        _assert_records(ev.records(), _ref(name, letterbox))
        _assert_result(ev.compute(), _ref(name, letterbox))


@pytest.mark.parametrize("name", ["nc3_m100", "nc80_m100"])
def test_three_updates_equal_one(name):
    one, three = _evaluate(name, True), _evaluate(name, True, splits=[(0, 2), (2, 3), (3, 5)])
    a, b = one.records(), three.records()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    ra, rb = one.compute(), three.compute()
    assert np.array_equal(ra["precision"], rb["precision"]) and np.array_equal(ra["recall"], rb["recall"]) and ra["stats"] == rb["stats"]
    assert np.array_equal(one.n_gt_ka, three.n_gt_ka)


def test_the_same_run_twice_gives_the_same_bytes_in_every_input_form():
    runs = [_evaluate("nc80_m100", True, form=f).records() for f in ("padded", "padded", "list", "copies")]
    for other in runs[1:]:
        for k in runs[0]:
            assert runs[0][k].tobytes() == other[k].tobytes(), k


def test_records_grow_past_the_first_capacity():
    from dyk.evalmap import CocoEvaluator
    c = _case("nc3_m100")
    ev = CocoEvaluator(c["nc"])
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    out, tg = torch.from_numpy(out).cuda(), _sub_targets(c["labels"])
    reps = 1024 // sum(counts) + 2
    for _ in range(reps):
        ev.update((out, counts), tg, c["shapes"])
    rec, r = ev.records(), _ref("nc3_m100")
    n = sum(counts)
    assert rec["conf"].shape[0] == reps * n > 1024
    for i in (0, reps - 1):
        s = slice(i * n, (i + 1) * n)
        assert np.array_equal(rec["dtm"][s], r["records"]["dtm"]) and np.array_equal(rec["dtig"][s], r["records"]["dtig"])
        assert np.array_equal(rec["img"][s], r["records"]["img"] + 5 * i)
        m = r["match_global"].copy()
        m[m >= 0] += i * tg.shape[0]
        assert np.array_equal(rec["match"][s], m)


SENT_F, SENT_I = -12345.5, -77
OUT_FIELDS = {"conf": (torch.float32, ()), "cls": (torch.int32, ()), "img": (torch.int32, ()), "rank": (torch.int32, ()),
              "box": (torch.float32, (4,)), "darea": (torch.float64, ()), "dtm": (torch.int32, "A"), "dtig": (torch.int32, "A"),
              "match": (torch.int16, "AT")}


def _direct(c, rec_off, cap, counts=None, **over):
    """one direct launch into sentinel-filled arrays -> (return code, host arrays, error words)"""
    from dyk import lib as L
    thr, areas, max_dets = _params(c)
    T, A = len(thr), len(areas)
    out, cnt = MC.padded_of(c["dets"], c["max_num"], SENT_F)
    cnt = cnt if counts is None else counts
    keep = {"out": torch.from_numpy(out).cuda(), "counts": torch.tensor(cnt, dtype=torch.int32).cuda(),
            "rec_off": torch.tensor(rec_off, dtype=torch.int32).cuda(), "targets": _sub_targets(c["labels"]),
            "gt_off": torch.tensor(np.concatenate(([0], np.cumsum([l.shape[0] for l in c["labels"]]))), dtype=torch.int32).cuda(),
            "shape0": torch.tensor(c["shapes"], dtype=torch.int32).cuda(), "err": torch.zeros(2, dtype=torch.int32).cuda()}
    for k, (dt, tail) in OUT_FIELDS.items():
        tail = {"A": (A,), "AT": (A, T)}.get(tail, tail)
        keep[k] = torch.full((cap,) + tail, SENT_F if dt.is_floating_point else SENT_I, dtype=dt).cuda()
    d = L.DykEvalCocoDesc()
    for k, v in keep.items():
        setattr(d, k, v.data_ptr())
    d.unpad = None
    for t, v in enumerate(thr):
        d.thr[t] = v
    for a, (lo, hi) in enumerate(areas):
        d.area[a][0], d.area[a][1] = lo, hi
    d.B, d.max_num, d.nt, d.nc, d.T, d.rec_cap = len(cnt), c["max_num"], keep["targets"].shape[0], c["nc"], T, cap
    d.A, d.max_det, d.round_boxes, d.img_base = A, max(max_dets), 1, 40
    for k, v in over.items():
        setattr(d, k, v)
    rc = L.load().dyk_eval_match_coco(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: keep[k].cpu().numpy() for k in OUT_FIELDS}, keep["err"].cpu().tolist()


@pytest.mark.parametrize("name", ["nc3_m8", "nc1_m160"])
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
        for k in ("cls", "rank", "match"):
            assert np.array_equal(got[k][s], want[k][w]), k
        for k in ("dtm", "dtig"):
            assert np.array_equal(got[k][s].view(np.uint32), want[k][w]), k
        assert np.array_equal(got["img"][s], want["img"][w] + 40)
        for k in FLOAT_FIELDS:
            assert np.array_equal(_bits(got[k][s]), _bits(want[k][w])), k
        first += n
    for k, (dt, _) in OUT_FIELDS.items():
        assert (got[k][~written] == (SENT_F if dt.is_floating_point else SENT_I)).all(), k
    minus = [-1 if b == 1 else n for b, n in enumerate(counts)]
    rc, got, err = _direct(c, rec_off, cap, counts=minus)
    s = slice(rec_off[0] + counts[0], rec_off[2])
    assert rc == 0 and all((got[k][s] == (SENT_F if dt.is_floating_point else SENT_I)).all() for k, (dt, _) in OUT_FIELDS.items())


def test_the_kernel_refuses_tables_that_leave_the_arrays():
    """records past rec_cap: the image writes nothing and the second error word is set (no out-of-bounds store); the
    argument errors are returned before any launch"""
    from dyk import lib as L
    c = _case("nc1_m8")
    counts = [0 if d is None else d.shape[0] for d in c["dets"]]
    rec_off = [0, 8, 16, 24, 32]
    assert counts[4] > 1
    rc, got, err = _direct(c, rec_off, cap=rec_off[4] + counts[4] - 1)        # the last record of image 4 does not fit
    assert rc == 0 and err == [0, 1]
    for k, (dt, _) in OUT_FIELDS.items():
        assert (got[k][rec_off[4]:] == (SENT_F if dt.is_floating_point else SENT_I)).all(), k
    assert (got["cls"][rec_off[2]:rec_off[2] + counts[2]] != SENT_I).all()
    for over in ({"T": 17}, {"T": 0}, {"A": 0}, {"A": 5}, {"max_det": 0}, {"max_num": L.EVAL_COCO_MAX_NUM + 1}, {"nc": 0}, {"B": 0},
                 {"dtig": None}, {"rank": None}):
        assert _direct(c, rec_off, 64, **over)[0] == -1, over
    assert L.load().dyk_eval_match_coco(None, None) == -1


def test_a_class_outside_the_range_sets_the_flag_and_matches_nothing():
    from dyk.evalmap import CocoEvaluator
    c = _case("nc3_m100")                                # the case's detections carry class 2
    rc, got, err = _direct(c, [0, 100, 200, 300, 400], 512, nc=2)
    want = _ref("nc3_m100")["records"]
    bad = want["cls"] == 2
    rows = np.concatenate([np.arange(100 * b, 100 * b + (0 if d is None else d.shape[0])) for b, d in enumerate(c["dets"])])
    assert rc == 0 and err == [1, 0] and bad.any()
    assert (got["dtm"][rows][bad] == 0).all() and (got["dtig"][rows][bad] == 0).all() and (got["match"][rows][bad] == -1).all()
    assert np.array_equal(got["dtm"][rows][~bad].view(np.uint32), want["dtm"][~bad]) and np.array_equal(got["rank"][rows], want["rank"])
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    ev = CocoEvaluator(2)
    ev.update((torch.from_numpy(out).cuda(), counts), torch.zeros((0, 6), device="cuda"), c["shapes"])
    with pytest.raises(ValueError, match="class"):
        ev.compute()
    ev.reset()
    assert ev.compute()["stats"] == [-1.0] * 12


def test_refusals():
    from dyk import lib as L
    from dyk.evalmap import CocoEvaluator
    c = _case("nc3_m100")
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    out, tg = torch.from_numpy(out).cuda(), _sub_targets(c["labels"])
    ev = CocoEvaluator(3)
    with pytest.raises(L.DykError):
        ev.update((out.cpu(), counts), tg, c["shapes"])
    with pytest.raises(L.DykError):
        ev.update((out, counts), tg.cpu(), c["shapes"])
    crowded = torch.zeros((1025, 6), device="cuda")
    crowded[:, 0] = 3
    crowded[:, 2:] = 0.1
    with pytest.raises(ValueError, match="image 3 .*1025"):
        ev.update((out, counts), crowded, c["shapes"])
    with pytest.raises(ValueError, match="sorted"):
        ev.update((out, counts), tg.flip(0), c["shapes"])
    wide = torch.zeros((5, L.EVAL_COCO_MAX_NUM + 1, 6), device="cuda")
    with pytest.raises(ValueError, match="513.*512"):
        ev.update((wide, counts), tg, c["shapes"])
    assert ev.num_imgs == 0 and ev.n_gt_ka.sum() == 0 and ev.records()["conf"].shape[0] == 0     # a refused batch leaves no trace


def test_the_64_pair_fixture_end_to_end(tiles):
    """the detections of the 64-pair fixture (tests/test_eval_ap.py: _state5, fp32, 910 of them) through the evaluator: the
    twelve stats equal coco_ref's on the same detections after scale_coords(...).round() on the host, in one update and batch
    by batch.  The numbers are printed, not pinned: there is no pycocotools to pin them against."""
    import test_eval_ap as TE
    from build_utils.parse_config import materialize_cfg
    from build_utils.utils import non_max_suppression, scale_coords
    from dyk.evalmap import CocoEvaluator
    from models import YOLO
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
    shapes = [(R5.SHAPE0[1], R5.SHAPE0[0])] * 64
    host = []
    for p in dets:
        if p is None:
            host.append(None)
            continue
        boxes = scale_coords((R5.H, R5.W), p[:, :4].clone(), R5.SHAPE0, R5.RATIO_PAD).round()
        host.append(np.concatenate([boxes.cpu().numpy(), p[:, 4:6].cpu().numpy()], 1).astype(np.float32))
    tn = targets.numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
    labels = [tn[tn[:, 0] == b][:, 1:].astype(np.float32) for b in range(64)]
    want = coco_ref.evaluate(host, labels, shapes, 1)
    ev = CocoEvaluator(1)
    ev.update(dets, targets.cuda(), shapes, img1_shape=(R5.H, R5.W), ratio_pad=R5.RATIO_PAD)
    res = ev.compute()
    print("64-pair fixture, COCO protocol, %d records:\n%s" % (ev.records()["conf"].shape[0], res["summary"]))
    print("stats", ["%.6f" % s for s in res["stats"]])
    _assert_records(ev.records(), want)
    _assert_result(res, want)
    assert ev.records()["conf"].shape[0] == int(TE.GOLD5["ndet"].sum()) == 910
    ev.reset()
    for c in range(0, 64, 16):                          # batch by batch, as an evaluation loop feeds it
        tb = targets[(targets[:, 0] >= c) & (targets[:, 0] < c + 16)].clone()
        tb[:, 0] -= c
        ev.update(dets[c:c + 16], tb.cuda(), shapes[c:c + 16], img1_shape=(R5.H, R5.W), ratio_pad=R5.RATIO_PAD)
    again = ev.compute()
    assert again["stats"] == res["stats"] and np.array_equal(again["precision"], res["precision"])
    _assert_records(ev.records(), want)
