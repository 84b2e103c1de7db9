"""merge-NMS on the GPU (dyk_nms_ex with DYK_NMS_MERGE; reference build_utils/utils.py:398, :450-454).

Reference of every test: the fp64-weighted restatement of tests/nms_merge_ref.py on the same `pred` on the host -- membership
in fp32 as the reference evaluates it, weights and sums in fp64, one rounding.  Coordinate bound: 2^-23 * max(|ref|, 1) (the
kernel's result contract in include/dyk_hip.h: the exact weighted mean of the fp32 inputs to one fp32 rounding; the reference
is that mean to one rounding too, so the two are at most two half-ulps = 2^-23 relative apart).  Scores, classes, counts and
rows must equal the plain call of the same build exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN

sys.path.insert(0, GOLDEN)
import cases  # noqa: E402
import nms_merge_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _kw(case):
    return dict(conf_thres=case["conf"], iou_thres=case["iou"], multi_label=case["multi"], classes=case["classes"],
                agnostic=case["agnostic"])


def _check(pred, what, **kw):
    """merged GPU output against the fp64-weighted restatement and against the plain GPU call; returns (merged, plain, info)."""
    from dyk import detect
    info = {}
    want, want_rows = ref.non_max_suppression(pred, merge=True, mode="fp64", info=info, **kw)
    dev = pred.cuda()
    got, rows = detect.non_max_suppression(dev, return_rows=True, merge=True, **kw)
    plain, prows = detect.non_max_suppression(dev, return_rows=True, merge=False, **kw)
    worst = 0.0
    for b in range(pred.shape[0]):
        if want[b] is None:
            assert got[b] is None and plain[b] is None and rows[b] is None, (what, b)
            continue
        g, p, w = got[b].cpu(), plain[b].cpu(), want[b]
        assert g.shape == p.shape == w.shape, (what, b, g.shape, p.shape, w.shape)
        assert torch.equal(g[:, 4:], p[:, 4:]) and torch.equal(g[:, 4:], w[:, 4:]), (what, b)     # conf, cls, order, count
        assert torch.equal(rows[b].cpu(), prows[b].cpu()) and rows[b].cpu().tolist() == want_rows[b].tolist(), (what, b)
        if not 1 < info["n"][b] < 3000:                                                           # :450
            assert torch.equal(g, p), (what, b, info["n"][b])
        err = (g[:, :4].double() - w[:, :4].double()).abs()
        bound = 2.0 ** -23 * w[:, :4].double().abs().clamp(min=1.0)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (what, b, float((err / bound).max()))
    print("%s: n %s, largest cluster %s, worst coordinate error %.3f of the bound" % (what, info["n"], info["cluster"], worst))
    return got, plain, info


@pytest.mark.parametrize("case", cases.nms_cases(), ids=lambda c: c["name"])
def test_merge_on_every_nms_case(case):
    got, plain, info = _check(cases.nms_pred(case), case["name"], **_kw(case))
    if case["name"] == "dense":                      # n = 20 160: no merge, the plain output bit for bit (checked in _check)
        assert info["n"] == [20160]
    if case["name"] == "sparse":                     # the merge moves boxes here, and more than 16 boxes are kept (wavefronts wrap)
        assert got[0].shape[0] > 16 and not torch.equal(got[0], plain[0])
    if case["name"] == "nc2_multi":                  # image 1 is cut at max_num = 100
        assert got[1].shape[0] == 100


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2999, 3000])
def test_merge_at_boundary_candidate_counts(n):
    pred = ref.cluster_rows(1, n, 100 + n)
    got, plain, info = _check(pred, "n=%d" % n, conf_thres=0.25, iou_thres=0.6, multi_label=False)
    assert info["n"] == [n]
    if n in (1, 3000):
        assert torch.equal(got[0], plain[0])
    else:
        assert not torch.equal(got[0], plain[0])
    if n >= 2999:
        assert got[0].shape[0] == 100


def test_merge_in_a_batch_whose_middle_image_is_empty():
    pred = ref.cluster_rows(3, 65, 7)
    pred[1, :, 4] = 0.0
    got, plain, info = _check(pred, "empty middle image", conf_thres=0.25, iou_thres=0.6, multi_label=False)
    assert info["n"] == [65, 0, 65] and got[1] is None and got[0] is not None and got[2] is not None


def _boxes(xyxy, scores, cls_probs=None):
    b = torch.tensor(xyxy, dtype=torch.float32)
    nc = 1 if cls_probs is None else len(cls_probs[0])
    p = torch.zeros(1, b.shape[0], 5 + nc)
    p[0, :, 0], p[0, :, 1] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    p[0, :, 2], p[0, :, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    p[0, :, 4] = torch.tensor(scores)
    p[0, :, 5:] = 1.0 if cls_probs is None else torch.tensor(cls_probs)
    return p


def _mean(boxes, scores):
    w = np.asarray(scores, dtype=np.float32).astype(np.float64)
    return ((w[:, None] * np.asarray(boxes, dtype=np.float64)).sum(0) / w.sum()).astype(np.float32)


def test_iou_equal_to_the_threshold_neither_suppresses_nor_joins():
    """[6,6,14,14] and [6,6,14,22]: inter 64, union 128, IoU exactly 0.5 -- `>` is strict in the suppression AND in the membership.
    [5,6,13,14] overlaps the first by 56/72 (suppressed, joins it) and the second by 56/136 (does not)."""
    bx = [[6, 6, 14, 14], [6, 6, 14, 22], [5, 6, 13, 14]]
    sc = [0.9, 0.8, 0.7]
    got, plain, _ = _check(_boxes(bx, sc), "threshold equality", conf_thres=0.1, iou_thres=0.5, multi_label=False)
    g = got[0].cpu().numpy()
    assert g.shape[0] == 2
    assert np.array_equal(g[1, :4], np.float32(bx[1]))                       # alone in its cluster: w * x / w is exact
    assert np.array_equal(g[0, :4], _mean([bx[0], bx[2]], [sc[0], sc[2]])) and g[0, 0] < 6.0
    assert np.array_equal(plain[0].cpu().numpy()[:, :4], np.float32(bx[:2]))


def test_class_offset_separates_the_clusters_unless_agnostic():
    """nc = 2, two candidates of different classes on (nearly: 2 px apart, so a merge shows) the same pixels."""
    bx = [[10, 10, 50, 50], [12, 10, 52, 50]]
    pred = _boxes(bx, [1.0, 1.0], cls_probs=[[0.9, 0.2], [0.3, 0.8]])
    kw = dict(conf_thres=0.25, iou_thres=0.6, multi_label=False)
    got, plain, _ = _check(pred, "class offset", agnostic=False, **kw)
    assert got[0].shape[0] == 2 and torch.equal(got[0], plain[0])            # one-member clusters: unchanged bit for bit
    got, plain, _ = _check(pred, "class offset, agnostic", agnostic=True, **kw)
    g = got[0].cpu().numpy()
    assert g.shape[0] == 1 and g[0, 5] == 0.0
    assert np.array_equal(g[0, :4], _mean(bx, [0.9, 0.8])) and g[0, 0] > 10.0


def test_two_runs_are_bit_identical():
    from dyk import detect
    case = [c for c in cases.nms_cases() if c["name"] == "nc2_multi"][0]
    for pred, kw in ((cases.nms_pred(case), _kw(case)),
                     (ref.cluster_rows(2, 2999, 5), dict(conf_thres=0.25, iou_thres=0.6, multi_label=False))):
        dev = pred.cuda()
        a = detect.non_max_suppression(dev, merge=True, **kw)
        junk = torch.full((1 << 20,), float("nan"), device="cuda")       # the second run's workspace starts from other bits
        del junk
        b = detect.non_max_suppression(dev, merge=True, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def _direct(pred, entry, flags, **kw):
    """dyk_nms / dyk_nms_ex through ctypes with a hand-built descriptor -> (return code, per-image outputs)"""
    from dyk import lib as L
    h = L.load()
    pred = pred.cuda().contiguous()
    B, N, no = pred.shape
    per = int(h.dyk_nms_workspace_bytes(N, no, 0))
    ws = torch.empty(B * per, dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, 100, 6), device="cuda")
    rows = torch.zeros((B, 100), dtype=torch.int32, device="cuda")
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    d = L.DykNmsDesc()
    d.pred, d.out, d.out_rows, d.counts, d.ws, d.ws_per_image = pred.data_ptr(), out.data_ptr(), rows.data_ptr(), counts.data_ptr(), ws.data_ptr(), per
    d.B, d.N, d.no, d.conf_thres, d.iou_thres = B, N, no, kw["conf_thres"], kw["iou_thres"]
    d.multi_label, d.agnostic, d.max_num, d.n_classes = 0, 0, 100, 0
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = h.dyk_nms(ctypes.byref(d), s) if entry == "dyk_nms" else h.dyk_nms_ex(ctypes.byref(d), flags, s)
    cnt = counts.cpu().tolist()
    return rc, [out[b, :n].cpu() for b, n in enumerate(cnt)]


def test_merge_off_is_the_plain_call_and_the_environment_switch(monkeypatch):
    from build_utils.utils import non_max_suppression as api
    from dyk import detect
    gold = np.load(os.path.join(GOLDEN, "nms.npz"))
    case = cases.nms_cases()[0]                                              # "sparse": nc = 1, multi_label off
    pred, kw = cases.nms_pred(case), _kw(case)
    dev = pred.cuda()
    want = [gold["%s|%d" % (case["name"], b)] for b in range(case["B"])]      # the reference's own output: the bits "as before"
    arr = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
    same = lambda res, exp: all(np.array_equal(arr(r), arr(e)) for r, e in zip(res, exp))
    monkeypatch.delenv("DYK_NMS_MERGE", raising=False)
    assert same(detect.non_max_suppression(dev, merge=False, **kw), want)
    assert same(detect.non_max_suppression(dev, merge=None, **kw), want)
    assert same(detect.non_max_suppression(dev, **kw), want) and same(api(dev, **kw), want)
    rc, out = _direct(pred, "dyk_nms", 0, **kw)
    assert rc == 0 and same(out, want)
    rc, out = _direct(pred, "dyk_nms_ex", 0, **kw)
    assert rc == 0 and same(out, want)
    rc, _ = _direct(pred, "dyk_nms_ex", 2, **kw)                             # unknown flag bit on a valid descriptor
    assert rc == -1
    merged = [m.cpu().numpy() for m in detect.non_max_suppression(dev, merge=True, **kw)]
    assert not same(merged, want)
    rc, out = _direct(pred, "dyk_nms_ex", 1, **kw)
    assert rc == 0 and same(out, merged)
    assert same(api(dev, merge=True, **kw), merged)
    monkeypatch.setenv("DYK_NMS_MERGE", "1")
    assert same(detect.non_max_suppression(dev, merge=None, **kw), merged) and same(api(dev, **kw), merged)
    assert same(detect.non_max_suppression(dev, merge=False, **kw), want) and same(api(dev, merge=False, **kw), want)
    monkeypatch.setenv("DYK_NMS_MERGE", "0")
    assert same(detect.non_max_suppression(dev, **kw), want)
    assert same(detect.non_max_suppression(dev, merge=True, **kw), merged)


def test_merged_eval_chain_on_the_64_pair_fixture(tiles):
    """fp32, pinned tiles (DYK_AUTOTUNE=0), as test_hip_eval_chain_matches_the_64_pair_reference_ap: the merged detections equal
    the restatement applied to the GPU's own `io` (bounds above), AP / LAMR equal that restatement's to 1e-9, and AP lies within
    the 1e-3 that test allows the plain fp32 AP, measured from the merged CPU value 0.7560124325."""
    import test_eval_ap as E
    from build_utils.parse_config import materialize_cfg
    from build_utils.utils import non_max_suppression, scale_coords
    from models import YOLO
    from oracle import metrics as ometrics, nms as onms
    from other_utils.metrics import compute_ap_lamr
    assert tiles == "pinned"
    R5 = E.R5
    _, sd = E._state5()
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(R5.CFG))
    m.load_state_dict(sd)
    m.dyk_dtype = "fp32"
    m = m.cuda().eval()
    v, l, targets = R5.dataset()
    with torch.no_grad():
        io = torch.cat([m(v[c:c + 16].cuda().float() / 255.0, l[c:c + 16].cuda().float() / 255.0)[0].clone() for c in range(0, 64, 16)])
    kw = dict(conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
    _check(io.cpu(), "64-pair fixture", **kw)
    dets = non_max_suppression(io, merge=True, **kw)
    plain = non_max_suppression(io, **kw)
    want, _ = ref.non_max_suppression(io.cpu(), merge=True, mode="fp64", **kw)
    res, ndet = E._ap5(dets, scale_coords, compute_ap_lamr, targets)
    res_p, ndet_p = E._ap5(plain, scale_coords, compute_ap_lamr, targets)
    res_w, ndet_w = E._ap5(want, onms.scale_coords, ometrics.compute_ap_lamr, targets)
    print("64-pair fixture, fp32, merged: AP %.10f LAMR %.10f %d detections | restatement on the same io: AP %.10f LAMR %.10f %d | "
          "plain: AP %.10f LAMR %.10f %d | CPU values on the recorded io: merged AP 0.7560124325, plain AP %.10f"
          % (res["ap"], res["lamr"], ndet, res_w["ap"], res_w["lamr"], ndet_w, res_p["ap"], res_p["lamr"], ndet_p, float(E.GOLD5["ap"])))
    assert ndet == ndet_w == ndet_p
    assert abs(res["ap"] - res_w["ap"]) <= 1e-9 and abs(res["lamr"] - res_w["lamr"]) <= 1e-9
    assert abs(res["ap"] - 0.7560124325) <= 1e-3
