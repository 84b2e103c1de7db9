"""The multi-class evaluator's host half against its yardstick, on the CPU (no GPU, no native library).

tests/map_ref.py runs compute_ap_lamr's sequential loop per class and threshold.  Here: with one class it IS
compute_ap_lamr (arrays equal, not close); other_utils.metrics.compute_map fed map_ref's records reproduces map_ref's AP and
LAMR exactly; a hand-computed case; score ties across images; and a list of wrong evaluators, each of which a named case of
tests/map_cases.py tells from the right one -- the case matrix has teeth."""
import numpy as np
import pytest

import map_cases as MC
import map_ref
from other_utils.metrics import _absolute_xyxy, box_iou, compute_ap_lamr, compute_map


def _ref(c):
    return map_ref.evaluate(c["dets"], c["labels"], c["shapes"], c["nc"], c["thresholds"])


def _compute(c, r):
    rec = r["records"]
    return compute_map(rec["conf"], rec["cls"], rec["tp_mask"], r["n_gt"], len(c["labels"]), c["thresholds"])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("name", ["nc1_t1_m8", "nc1_t10_m100_full", "ties_across_images"])
def test_one_class_is_compute_ap_lamr(name):
    """nc = 1, T = (0.5,), ground truth in every image: every array of compute_ap_lamr's result, equal"""
    c = dict(MC.HAND[name] if name in MC.HAND else MC.case(name))
    keep = [b for b, lab in enumerate(c["labels"]) if lab.shape[0]]
    labels, dets, shapes = [c["labels"][b] for b in keep], [c["dets"][b] for b in keep], [c["shapes"][b] for b in keep]
    preds = []
    for i, d in enumerate(dets):
        if d is not None:
            preds += [{"img_id": i, "conf": float(d[j, 4]), "bbox": d[j, :4]} for j in range(d.shape[0])]
    preds.sort(key=lambda q: q["conf"], reverse=True)
    want = compute_ap_lamr(preds, [lab.copy() for lab in labels], shapes)
    got = map_ref.evaluate(dets, labels, shapes, 1, (0.5,))
    assert got["ap"][0, 0] == want["ap"] and got["lamr"][0, 0] == want["lamr"]
    for k in ("recall", "precision", "fppi", "mr"):
        assert np.array_equal(got["curves"][0, 0][k], want[k]), k
    cm = compute_map(got["records"]["conf"], got["records"]["cls"], got["records"]["tp_mask"], got["n_gt"], len(labels), (0.5,))
    assert cm["ap"][0, 0] == want["ap"] and cm["lamr"][0, 0] == want["lamr"] and cm["map50"] == want["ap"]
    assert np.array_equal(cm["recall"][0][0], want["recall"]) and np.array_equal(cm["precision"][0][0], want["precision"])


@pytest.mark.parametrize("name", sorted(MC.MATRIX) + sorted(MC.HAND))
def test_compute_map_reproduces_the_reference_from_its_records(name):
    c = MC.HAND[name] if name in MC.HAND else MC.case(name)
    r = _ref(c)
    cm = _compute(c, r)
    assert _same(cm["ap"], r["ap"]) and _same(cm["lamr"], r["lamr"])
    has = r["n_gt"] > 0
    assert cm["map"] == float(r["ap"][has].mean())
    for (cl, t), cur in r["curves"].items():
        assert np.array_equal(cm["recall"][cl][t], cur["recall"]) and np.array_equal(cm["precision"][cl][t], cur["precision"])
    assert ("map50" in cm) == (0.5 in c["thresholds"])
    if name in MC.MATRIX:                               # the seeded cases exercise both outcomes
        assert 0 < int((r["records"]["tp_mask"] != 0).sum()) < r["records"]["conf"].shape[0]


def test_hand_computed_case():
    c = MC.HAND["hand_map"]
    r = _ref(c)
    assert r["records"]["tp_mask"].tolist() == [1, 0, 1] and r["records"]["match"].tolist() == [0, 0, 1]
    cm = compute_map(r["records"]["conf"], r["records"]["cls"], r["records"]["tp_mask"], r["n_gt"], 1, (0.5,), names=["a", "b", "c"])
    assert cm["ap"][0, 0] == pytest.approx(5 / 6, abs=1e-15) and cm["ap"][1, 0] == 0.0 and np.isnan(cm["ap"][2, 0])
    assert cm["lamr"][1, 0] == 1.0 and np.isnan(cm["lamr"][2, 0])
    assert cm["map50"] == pytest.approx(5 / 12, abs=1e-15) and cm["map"] == cm["map50"]
    assert [ln.split()[0] for ln in cm["summary"].splitlines()[1:4]] == ["a", "b", "c"]
    assert "coco" not in cm["summary"].lower()


def test_score_ties_across_images_keep_image_order():
    """four detections with conf 0.5 in two images: the stable sort keeps (image, rank); swapping the two images' records
    changes the curve, so the order is observable"""
    c = MC.HAND["ties_across_images"]
    r = _ref(c)
    rec = r["records"]
    assert rec["tp_mask"].tolist() == [1, 0, 0, 1, 0]
    cm = _compute(c, r)
    assert np.array_equal(cm["recall"][0][0], [0.5, 0.5, 0.5, 1.0, 1.0])
    swapped = np.array([3, 4, 0, 1, 2])
    other = compute_map(rec["conf"][swapped], rec["cls"][swapped], rec["tp_mask"][swapped], r["n_gt"], 2, (0.5,))
    assert not np.array_equal(other["recall"][0][0], cm["recall"][0][0])


def test_exact_half_and_twins():
    r = _ref(MC.HAND["exact_half"])
    assert r["records"]["iou"][0] == 0.5 and r["records"]["tp_mask"].tolist() == [1, 0] and r["records"]["iou"][1] < 0.5
    r = _ref(MC.HAND["twins"])
    assert r["records"]["match"].tolist() == [0, 0] and r["records"]["tp_mask"].tolist() == [1, 0]
    r = _ref(MC.HAND["other_class"])
    assert r["records"]["tp_mask"].tolist() == [0, 1, 0] and r["records"]["match"].tolist() == [-1, 0, -1]
    assert r["records"]["iou"].tolist() == [0.0, 1.0, 0.0]
    r = _ref(MC.HAND["per_threshold"])
    assert r["records"]["tp_mask"].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------------------------------
# mutants: one general matching loop with a switch per classic mistake; with every switch off it is the right evaluator
def _iou_without_plus1(b, g):
    w = np.clip(np.minimum(b[2], g[:, 2]) - np.maximum(b[0], g[:, 0]), 0, 1e5)
    h = np.clip(np.minimum(b[3], g[:, 3]) - np.maximum(b[1], g[:, 1]), 0, 1e5)
    return w * h / ((b[2] - b[0]) * (b[3] - b[1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - w * h)


def _matcher(c, second_best=False, strict=False, ignore_class=False, shared_claims=False, last_max=False, no_plus1=False):
    T = len(c["thresholds"])
    tp_mask, match = [], []
    row0 = 0
    for d, lab, (w, h) in zip(c["dets"], c["labels"], c["shapes"]):
        gt = _absolute_xyxy([lab], [(w, h)])[0][:, 1:].astype(np.int32)
        gcls = lab[:, 0].astype(np.int32)
        claimed = np.zeros((T, gt.shape[0]), dtype=bool)
        for j in range(0 if d is None else d.shape[0]):
            idx = np.arange(gt.shape[0]) if ignore_class else np.nonzero(gcls == int(d[j, 5]))[0]
            if idx.size == 0:
                tp_mask.append(0)
                match.append(-1)
                continue
            box = d[j:j + 1, :4]
            iou = _iou_without_plus1(box[0], gt[idx]) if no_plus1 else box_iou(box, gt[idx])[0]
            k = iou.shape[0] - 1 - int(np.argmax(iou[::-1])) if last_max else int(np.argmax(iou))
            m = 0
            for t, thr in enumerate(c["thresholds"]):
                row = claimed[0] if shared_claims else claimed[t]
                kk = k
                if second_best and row[idx[kk]]:
                    free = [q for q in np.argsort(-iou, kind="stable") if not row[idx[q]]]
                    kk = free[0] if free else k
                ok = iou[kk] > thr if strict else iou[kk] >= thr
                if ok and not row[idx[kk]]:
                    row[idx[kk]] = True
                    m |= 1 << t
            tp_mask.append(m)
            match.append(row0 + int(idx[k]))
        row0 += lab.shape[0]
    return np.array(tp_mask, np.uint32), np.array(match, np.int32)


MUTANTS = {
    "second_best": ("second_best", "a claimed best box falls back to the second best"),
    "strict": ("exact_half", "> instead of >="),
    "ignore_class": ("other_class", "the class column is ignored"),
    "shared_claims": ("per_threshold", "claimed bits shared by the thresholds"),
    "last_max": ("twins", "the last maximum instead of the first"),
    "no_plus1": ("exact_half", "extents without the pixel-inclusive +1"),
}


@pytest.mark.parametrize("name", sorted(MC.HAND) + ["nc3_t10_m100", "nc80_t16_m100"])
def test_the_unswitched_matcher_is_the_reference(name):
    c = MC.HAND[name] if name in MC.HAND else MC.case(name)
    tp, match = _matcher(c)
    rec = _ref(c)["records"]
    assert np.array_equal(tp, rec["tp_mask"]) and np.array_equal(match, rec["match"])


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_flagged_by_its_case(mutant):
    name, what = MUTANTS[mutant]
    c = MC.HAND[name]
    tp, match = _matcher(c, **{mutant: True})
    rec = _ref(c)["records"]
    assert not (np.array_equal(tp, rec["tp_mask"]) and np.array_equal(match, rec["match"])), what


def test_refusals_and_edges_of_compute_map():
    e = np.zeros(0)
    cm = compute_map(e.astype(np.float32), e.astype(np.int32), e.astype(np.uint32), [2, 0], 3, (0.5, 0.75))
    assert cm["ap"][0].tolist() == [0.0, 0.0] and np.isnan(cm["ap"][1]).all() and cm["map"] == 0.0 and cm["map50"] == 0.0
    cm = compute_map(e.astype(np.float32), e.astype(np.int32), e.astype(np.uint32), [0], 1, (0.75,))
    assert np.isnan(cm["map"]) and "map50" not in cm
