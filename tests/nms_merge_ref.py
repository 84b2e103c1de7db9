"""CPU restatement of the reference's merge-NMS stage (test infrastructure, written independently).

Reference build_utils/utils.py:450-454 (`merge`, a local setting that is False as shipped, :398) on top of
oracle.nms: after greedy suppression and the [:max_num] cut (:448-449), in images with 1 < n < 3000 candidates
(:450, both strict), every kept box k becomes

    sum_j w_kj * x[j, :4] / sum_j w_kj,   w_kj = (box_iou(boxes[i[k]], boxes[j]) > iou_thres) * score_j

with box_iou of :141-163 -- inter / (area_k + area_j - inter), inter = max(0, ..) * max(0, ..), fp32 -- taken on the
class-offset boxes of :447 as rounded, over ALL n candidates, and the mean taken over the un-offset corners of the
original candidates.  conf, cls, order and count are the plain output's.

Two forms of the weighted mean:
  * mode="fp32": the literal one -- fp32 weights, torch.mm in fp32, one fp32 division (:453-454);
  * mode="fp64": membership as above (fp32), weights and sums in fp64, one division, one rounding to fp32.  This is
    the exact weighted mean of the fp32 inputs to one rounding; the HIP kernel is held to it.
"""
import numpy as np
import torch

from oracle import nms as onms

MAX_WH = 4096                                                     # :399


def candidates(x, conf_thres, multi_label, classes):
    """One image [N, 5+nc] -> (cand [n,6] = x1,y1,x2,y2,conf,cls in row order, rows [n]) after every filter of
    :408-431, restated like oracle.nms.non_max_suppression does (which does not hand the candidates out)."""
    nc = x.shape[1] - 5
    multi_label = multi_label and nc > 1
    rows = torch.arange(x.shape[0])
    m = x[:, 4] > conf_thres
    x, rows = x[m], rows[m]
    m = ((x[:, 2:4] > 2) & (x[:, 2:4] < MAX_WH)).all(1)
    x, rows = x[m].clone(), rows[m]
    if not x.shape[0]:
        return torch.zeros(0, 6), rows
    x[:, 5:] *= x[:, 4:5]
    box = onms.xywh2xyxy(x[:, :4])
    if multi_label:
        i, j = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).t()
        c, rows = torch.cat((box[i], x[i, j + 5].unsqueeze(1), j.float().unsqueeze(1)), 1), rows[i]
    else:
        conf, j = x[:, 5:].max(1)
        k = conf > conf_thres
        c, rows = torch.cat((box, conf.unsqueeze(1), j.float().unsqueeze(1)), 1)[k], rows[k]
    if classes:
        k = (c[:, 5:6] == torch.tensor(classes, dtype=c.dtype)).any(1)
        c, rows = c[k], rows[k]
    return c, rows


def membership(kept_boxes, boxes, iou_thres):
    """box_iou(:141-163)(kept, all) > iou_thres in fp32, operation for operation: [k, n] bool."""
    a = kept_boxes.numpy().astype(np.float32)
    b = boxes.numpy().astype(np.float32)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2])
    wh = np.maximum(wh, np.float32(0))
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area_a[:, None] + area_b[None, :] - inter)
    assert iou.dtype == np.float32
    return iou > np.float32(iou_thres)


def merge_image(cand, iou_thres, agnostic, max_num, mode):
    """cand [n,6] in row order -> (out [k,6], keep [k] indices into cand, largest cluster size)."""
    n = cand.shape[0]
    c = cand[:, 5] * 0 if agnostic else cand[:, 5]                                     # :446
    boxes, scores = cand[:, :4].clone() + c.view(-1, 1) * MAX_WH, cand[:, 4]           # :447
    keep = torch.as_tensor(onms.nms_numpy(boxes.numpy(), scores.numpy(), iou_thres), dtype=torch.long)[:max_num]
    out = cand[keep].clone()
    cluster = 1
    if 1 < n < 3e3:                                                                    # :450
        member = membership(boxes[keep], boxes, iou_thres)                             # :452
        cluster = int(member.sum(1).max())
        if mode == "fp32":
            w = torch.from_numpy(member).float() * scores[None]                        # :453
            out[:, :4] = torch.mm(w, cand[:, :4]).float() / w.sum(1, keepdim=True)     # :454
        else:
            w = member.astype(np.float64) * scores.numpy().astype(np.float64)[None]
            with np.errstate(divide="ignore", invalid="ignore"):
                mean = (w @ cand[:, :4].numpy().astype(np.float64)) / w.sum(1, keepdims=True)
            out[:, :4] = torch.from_numpy(mean.astype(np.float32))
    return out, keep, cluster


def non_max_suppression(prediction, conf_thres=0.1, iou_thres=0.6, multi_label=True, classes=None, agnostic=False,
                        max_num=100, merge=True, mode="fp64", info=None):
    """oracle.nms.non_max_suppression with the merge stage.  Returns (out, rows): per image [k,6] / row of `prediction`
    each detection came from, or None.  merge=False is the plain output.  `info`, a dict, receives "n" (candidates per
    image) and "cluster" (largest cluster per image)."""
    prediction = prediction.detach().float().cpu()
    out, out_rows = [None] * prediction.shape[0], [None] * prediction.shape[0]
    ns, clusters = [], []
    for xi, x in enumerate(prediction):
        cand, rows = candidates(x, conf_thres, multi_label, classes)
        ns.append(cand.shape[0])
        clusters.append(0)
        if not cand.shape[0]:
            continue
        if merge:
            o, keep, clusters[-1] = merge_image(cand, iou_thres, agnostic, max_num, mode)
        else:
            c = cand[:, 5] * 0 if agnostic else cand[:, 5]
            boxes = cand[:, :4].clone() + c.view(-1, 1) * MAX_WH
            keep = torch.as_tensor(onms.nms_numpy(boxes.numpy(), cand[:, 4].numpy(), iou_thres), dtype=torch.long)[:max_num]
            o = cand[keep]
        out[xi], out_rows[xi] = o, rows[keep]
    if info is not None:
        info["n"], info["cluster"] = ns, clusters
    return out, out_rows


def cluster_rows(B, n, seed, ncl=None):
    """Seeded decoded predictions [B, n, 6] (cx, cy, w, h, obj, cls) whose rows ALL pass the filters at conf_thres <= 0.25
    (nc = 1: candidate count = n): ncl object clusters per image on a grid 200 px apart (so distinct clusters never overlap),
    members jittered by a few pixels around a common box -- every cluster has one survivor and the rest merge into it."""
    g = torch.Generator().manual_seed(seed)
    ncl = ncl or max(1, n // 8)
    side = int(np.ceil(np.sqrt(ncl)))
    which = torch.randint(0, ncl, (B, n), generator=g)
    w = torch.rand(B, ncl, generator=g) * 60 + 16
    h = torch.rand(B, ncl, generator=g) * 100 + 32
    jit = torch.randn(B, n, 4, generator=g) * torch.tensor([2.0, 2.0, 1.5, 3.0])
    p = torch.zeros(B, n, 6)
    p[..., 0] = (which % side).float() * 200 + 100 + jit[..., 0]
    p[..., 1] = (which // side).float() * 200 + 100 + jit[..., 1]
    p[..., 2] = (torch.gather(w, 1, which) + jit[..., 2]).clamp(min=4.0)
    p[..., 3] = (torch.gather(h, 1, which) + jit[..., 3]).clamp(min=4.0)
    p[..., 4] = torch.rand(B, n, generator=g) * 0.7 + 0.3
    p[..., 5] = 1.0
    return p
