"""The COCO-protocol evaluator without a GPU: the yardstick tests/coco_ref.py against the hand-worked answers of
tests/coco_cases.py and against its own coverage counters; other_utils.metrics.coco_accumulate against the yardstick's
plain accumulation (precision / recall EXACTLY: both are integer counts divided once; the stats within 1e-10: a mean of at
most 10 * 101 * 80 values in [0, 1], naive fp64 summation is bounded by n * 2^-53 ~ 9e-12); CocoEvaluator's ground-truth
counter; the descriptor's layout against gcc; the refusals that need no device."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import coco_cases as CC
import coco_ref
import map_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    return CC.HAND[name] if name in CC.HAND else CC.case(name)


def _params(c):
    return c.get("thresholds", coco_ref.THRESHOLDS), c.get("areas", coco_ref.AREAS), c.get("max_dets", coco_ref.MAX_DETS)


@functools.lru_cache(maxsize=None)
def _ref(name, round_boxes=True):
    c = _case(name)
    return coco_ref.evaluate(c["dets"], c["labels"], c["shapes"], c["nc"], *_params(c), round_boxes=round_boxes)


@pytest.mark.parametrize("round_boxes", [True, False])
@pytest.mark.parametrize("name", sorted(CC.HAND))
def test_hand_cases_have_their_written_answers(name, round_boxes):
    r = _ref(name, round_boxes)
    CC.check_hand(name, r["records"], r["stats"], r["npig"], round_boxes)


def test_twins_differ_from_the_voc_rule():
    """the case the two rules disagree on: two equal boxes, two detections -- both TP here, the second an FP under the
    arg-max rule of compute_map (tests/map_ref.py)"""
    import map_ref
    c = CC.HAND["twins"]
    voc = map_ref.evaluate(c["dets"], c["labels"], c["shapes"], 1, (0.5,))
    assert voc["records"]["tp_mask"].tolist() == [1, 0]
    assert (_ref("twins")["records"]["dtm"][:, 0] & 1).tolist() == [1, 1]


@pytest.mark.parametrize("name", sorted(CC.MATRIX))
def test_every_rule_is_exercised(name):
    k = _ref(name)["counters"]
    print(name, k)
    for a in (1, 2, 3):                                  # each restricted range holds ignored and kept boxes
        assert k["gt_ignored"][a] > 0 and k["gt_kept"][a] > 0
    assert k["matched_to_ignored"] > 0 and k["unmatched_ignored"] > 0
    if name in ("nc3_m100", "nc1_m160"):
        assert k["not_argmax"] > 0 and k["stopped_before_better_ignored"] > 0
    if name == "nc1_m160":
        assert k["rank_cut"] > 0
    assert k["iou_ties"] == 0                            # hence the hand case:
    assert _ref("twins")["counters"]["iou_ties"] > 0


@pytest.mark.parametrize("name", sorted(CC.MATRIX) + sorted(CC.HAND))
def test_accumulate_equals_the_plain_loops(name):
    from other_utils.metrics import coco_accumulate
    c, r = _case(name), _ref(name)
    rec = r["records"]
    thr, areas, max_dets = _params(c)
    got = coco_accumulate(rec["conf"], rec["cls"], rec["img"], rec["rank"], rec["dtm"], rec["dtig"], r["npig"], thr, areas, max_dets)
    assert got["precision"].shape == (len(thr), 101, c["nc"], len(areas), len(max_dets))
    assert np.array_equal(got["precision"], r["precision"]) and np.array_equal(got["recall"], r["recall"])
    assert len(got["stats"]) == 12 and np.abs(np.array(got["stats"]) - np.array(r["stats"])).max() <= 1e-10
    assert got["ap_per_class"].shape == (c["nc"],) and len(got["summary"].splitlines()) == 12


def test_accumulate_does_not_depend_on_record_order_within_an_image():
    """the records come in NMS order, not in rank order: shuffling them within an image changes nothing"""
    from other_utils.metrics import coco_accumulate
    r = _ref("nc3_m100")
    rec = r["records"]
    rng = np.random.default_rng(0)
    perm = np.concatenate([rng.permutation(np.nonzero(rec["img"] == b)[0]) for b in range(5)]).astype(np.int64)
    args = lambda p: [rec[k][p] for k in ("conf", "cls", "img", "rank", "dtm", "dtig")]
    a = coco_accumulate(*args(np.arange(perm.shape[0])), r["npig"], coco_ref.THRESHOLDS, coco_ref.AREAS, coco_ref.MAX_DETS)
    b = coco_accumulate(*args(perm), r["npig"], coco_ref.THRESHOLDS, coco_ref.AREAS, coco_ref.MAX_DETS)
    assert np.array_equal(a["precision"], b["precision"]) and a["stats"] == b["stats"]


def test_summary_lines_and_custom_parameters():
    from other_utils.metrics import coco_accumulate
    r = _ref("hand_ap")
    rec = r["records"]
    got = coco_accumulate(rec["conf"], rec["cls"], rec["img"], rec["rank"], rec["dtm"], rec["dtig"], r["npig"],
                          coco_ref.THRESHOLDS, coco_ref.AREAS, coco_ref.MAX_DETS, names=["person"])
    lines = got["summary"].splitlines()
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
    assert len(lines) == 13 and "person" in lines[12]
    # one area range, thresholds without 0.5 / 0.75: what does not exist is -1
    one = coco_ref.evaluate(CC.HAND["hand_ap"]["dets"], CC.HAND["hand_ap"]["labels"], [(128, 128)], 1, (0.6, 0.7), ((0.0, 1e10),), (100,))
    rec = one["records"]
    got = coco_accumulate(rec["conf"], rec["cls"], rec["img"], rec["rank"], rec["dtm"], rec["dtig"], one["npig"], (0.6, 0.7), ((0.0, 1e10),), (100,))
    assert got["stats"][1:6] == [-1.0] * 5 and got["stats"][7:] == [-1.0] * 5 and got["stats"][6] == 1.0
    assert np.abs(np.array(got["stats"]) - np.array(one["stats"])).max() <= 1e-10


@pytest.mark.parametrize("name", sorted(CC.MATRIX) + ["area_edges", "no_gt_class"])
def test_ground_truth_counter_equals_the_reference(name):
    from dyk.evalmap import CocoEvaluator
    c = _case(name)
    ev = CocoEvaluator(c["nc"])
    assert np.array_equal(ev.count_ground_truth(MC.targets_of(c["labels"]), c["shapes"]), _ref(name)["npig"])
    assert ev.n_gt_ka.shape == (c["nc"], 4) and ev.n_gt_ka.sum() == 0


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib as L
    cls = L.DykEvalCocoDesc
    names = [f[0] for f in cls._fields_]
    src = tmp_path / "probe.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(DykEvalCocoDesc));',
             'printf("limits %d\\n", DYK_EVAL_MAX_AREA * 10000 + DYK_EVAL_COCO_MAX_NUM);']
    lines += ['printf("%s %%zu\\n", offsetof(DykEvalCocoDesc, %s));' % (n, n) for n in names]
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls)
    for n in names:
        assert int(out[n]) == getattr(cls, n).offset, n
    assert int(out["limits"]) == L.EVAL_MAX_AREA * 10000 + L.EVAL_COCO_MAX_NUM and L.EVAL_MAX_AREA == 4
    assert L.load().dyk_abi_version() == 5 and L.load().dyk_eval_match_coco(None, None) == -1


def test_refusals_that_need_no_device():
    from dyk import lib as L
    from dyk.evalmap import CocoEvaluator
    with pytest.raises(ValueError, match="16 IoU thresholds.*17"):
        CocoEvaluator(1, [0.1 + 0.05 * i for i in range(17)])
    with pytest.raises(ValueError, match="4 area ranges.*5"):
        CocoEvaluator(1, area_ranges=[(0, 1e10)] * 5)
    CocoEvaluator(1, [0.1 + 0.05 * i for i in range(16)], area_ranges=[(0, 1e10)] * 4)     # 64 (area, threshold) pairs: the most
    with pytest.raises(ValueError, match="max_dets"):
        CocoEvaluator(1, max_dets=(10, 1))
    with pytest.raises(ValueError, match="nc"):
        CocoEvaluator(0)
    ev = CocoEvaluator(3)
    assert ev.iou_thresholds == coco_ref.THRESHOLDS and ev.area_ranges == coco_ref.AREAS and ev.max_dets == (1, 10, 100)
    c = CC.case("nc3_m100")
    out, counts = MC.padded_of(c["dets"], c["max_num"])
    with pytest.raises(L.DykError, match="no CPU"):
        ev.update((torch.from_numpy(out), counts), torch.from_numpy(MC.targets_of(c["labels"])), c["shapes"])
    assert ev.num_imgs == 0 and ev.n_gt_ka.sum() == 0 and ev.records()["match"].shape == (0, 4, 10)
    res = ev.compute()                                   # nothing seen: every stat is -1
    assert res["stats"] == [-1.0] * 12 and res["precision"].shape == (10, 101, 3, 4, 3)
