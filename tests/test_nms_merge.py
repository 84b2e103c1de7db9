"""merge-NMS (reference build_utils/utils.py:398, :450-454) on the CPU: the restatement of tests/nms_merge_ref.py against the
recorded values of the 64-pair fixture, its literal fp32 form against its fp64-weighted form on every nms case, and the C ABI of
dyk_nms_ex.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import torch

from helpers import GOLDEN

sys.path.insert(0, GOLDEN)
import cases  # noqa: E402
import nms_merge_ref as ref  # noqa: E402


def _kw(case):
    return dict(conf_thres=case["conf"], iou_thres=case["iou"], multi_label=case["multi"], classes=case["classes"],
                agnostic=case["agnostic"])


def test_restatement_reproduces_the_fixture_numbers():
    """tests/golden/evalap_trained64.npz `io`, conf 0.1 / IoU 0.6, multi_label=False.  Plain: the reference's recorded AP / LAMR /
    910 detections.  Merged (measured on the CPU with this restatement): AP 0.7560124325, LAMR 0.4836055601, same count, scores,
    classes and order."""
    import test_eval_ap as E
    from oracle import metrics as ometrics, nms as onms
    R5, GOLD5 = E.R5, E.GOLD5
    io = torch.from_numpy(GOLD5["io"])
    _, _, targets = R5.dataset()
    kw = dict(conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
    info = {}
    plain, prow = ref.non_max_suppression(io, merge=False, **kw)
    merged, mrow = ref.non_max_suppression(io, merge=True, mode="fp32", info=info, **kw)
    merged64, _ = ref.non_max_suppression(io, merge=True, mode="fp64", **kw)
    oracle = onms.non_max_suppression(io, **kw)
    move, gap = 0.0, 0.0
    for a, b, c, o, ra, rb in zip(plain, merged, merged64, oracle, prow, mrow):
        if o is None:                                              # (one image of the fixture has no candidate)
            assert a is None and b is None and c is None
            continue
        assert torch.equal(a, o)                                   # the restatement's plain leg IS oracle.nms
        assert torch.equal(a[:, 4:], b[:, 4:]) and torch.equal(ra, rb) and a.shape == b.shape
        move = max(move, float((a[:, :4] - b[:, :4]).abs().max()))
        gap = max(gap, float((b[:, :4] - c[:, :4]).abs().max()))
    res_p, n_p = E._ap5(plain, onms.scale_coords, ometrics.compute_ap_lamr, targets)
    res_m, n_m = E._ap5(merged, onms.scale_coords, ometrics.compute_ap_lamr, targets)
    res_64, _ = E._ap5(merged64, onms.scale_coords, ometrics.compute_ap_lamr, targets)
    print("plain AP %.10f LAMR %.10f %d | merged AP %.10f LAMR %.10f %d | fp64-weighted AP %.10f | boxes move by up to %.3f px, "
          "fp32 vs fp64 form %.3g px | n per image %d..%d, largest cluster %d"
          % (res_p["ap"], res_p["lamr"], n_p, res_m["ap"], res_m["lamr"], n_m, res_64["ap"], move, gap, min(n for n in info["n"] if n),
             max(info["n"]), max(info["cluster"])))
    assert n_p == n_m == int(GOLD5["ndet"].sum()) == 910
    assert abs(res_p["ap"] - float(GOLD5["ap"])) < 1e-6 and abs(res_p["lamr"] - float(GOLD5["lamr"])) < 1e-6
    assert abs(res_m["ap"] - 0.7560124325) < 1e-6 and abs(res_m["lamr"] - 0.4836055601) < 1e-6
    assert abs(res_64["ap"] - res_m["ap"]) < 1e-9
    assert move > 1.0                                              # the merge does something here


def test_fp32_and_fp64_forms_agree_on_every_nms_case():
    """The literal fp32 form (fp32 weights, torch.mm, :453-454) and the fp64-weighted form differ by at most
    (m + 2) * 2^-24 * max|coord| with m the largest cluster of the case: m products rounded once each and m - 1 fp32 additions in
    the numerator, the fp32 weight sum, the division and the final rounding of the fp64 form, each at most 2^-24 relative to a
    partial sum that is bounded by the result's scale (weights are positive), up to the (1 + 2^-24)^m second-order terms."""
    for case in cases.nms_cases():
        pred = cases.nms_pred(case)
        info = {}
        plain, _ = ref.non_max_suppression(pred, merge=False, **_kw(case))
        a, ra = ref.non_max_suppression(pred, merge=True, mode="fp32", info=info, **_kw(case))
        b, rb = ref.non_max_suppression(pred, merge=True, mode="fp64", **_kw(case))
        m, diff, scale = max(info["cluster"]), 0.0, 0.0
        for img in range(case["B"]):
            if plain[img] is None:
                assert a[img] is None and b[img] is None
                continue
            assert torch.equal(ra[img], rb[img])
            assert torch.equal(a[img][:, 4:], plain[img][:, 4:]) and torch.equal(b[img][:, 4:], plain[img][:, 4:])
            if not 1 < info["n"][img] < 3000:                      # :450: no merge, bit for bit the plain output
                assert torch.equal(a[img], plain[img]) and torch.equal(b[img], plain[img])
            diff = max(diff, float((a[img][:, :4] - b[img][:, :4]).abs().max()))
            scale = max(scale, float(b[img][:, :4].abs().max()))
        bound = (m + 2) * 2.0 ** -24 * scale
        print("%-14s n %s largest cluster %d: fp32 vs fp64 form %.3g, bound %.3g" % (case["name"], info["n"], m, diff, bound))
        assert diff <= bound, (case["name"], diff, bound)
        if case["name"] == "dense":
            assert info["n"] == [20160]
        if case["name"] == "sparse":
            assert m > 3 and diff > 0                              # the case exercises the merge


def test_abi_of_dyk_nms_ex():
    from dyk import lib
    h = lib.load()
    assert hasattr(h, "dyk_nms_ex") and lib.NMS_MERGE == 1
    assert h.dyk_nms_ex(None, 0, None) == -1                       # DYK_ERR_ARG
    assert h.dyk_nms_ex(None, lib.NMS_MERGE, None) == -1
    d = lib.DykNmsDesc()
    assert h.dyk_nms_ex(ctypes.byref(d), 2, None) == -1            # unknown flag bit
    assert h.dyk_nms_ex(ctypes.byref(d), lib.NMS_MERGE | 4, None) == -1
    assert h.dyk_nms_ex(ctypes.byref(d), lib.NMS_MERGE, None) == -1   # null pointers inside
    assert h.dyk_abi_version() == 5
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "dyk_hip.h")).read()
    assert "#define DYK_NMS_MERGE 1" in hdr
