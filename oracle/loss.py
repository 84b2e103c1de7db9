"""Oracle (test infrastructure): target assignment and YOLO loss on the CPU, fp32 / int64.

Restates reference build_utils/utils.py:95-138 (bbox_iou), :166-171 (wh_iou), :209-293
(compute_loss) and :296-384 (build_targets).  Pinned by tests/golden/targets_*.npz and
loss_*.npz generated from the reference (tests/golden/make_golden.py).
"""
import math

import torch
import torch.nn.functional as F


def wh_iou(wh1, wh2):
    """utils.py:166-171: IoU of boxes sharing a corner; wh1 [n,2], wh2 [m,2] -> [n,m]."""
    a = wh1[:, None]
    b = wh2[None]
    inter = torch.min(a, b).prod(2)
    return inter / (a.prod(2) + b.prod(2) - inter)


def bbox_iou_xywh(box1, box2, kind="ciou", detach_alpha=True, aux=None):
    """utils.py:95-138 with x1y1x2y2=False.  box1 [4,n] (cx,cy,w,h rows), box2 [n,4].  detach_alpha=False is a deliberate
    mistake (loss_reference); aux: a dict that receives the intersection areas."""
    box2 = box2.t()
    b1_x1, b1_x2 = box1[0] - box1[2] / 2, box1[0] + box1[2] / 2
    b1_y1, b1_y2 = box1[1] - box1[3] / 2, box1[1] + box1[3] / 2
    b2_x1, b2_x2 = box2[0] - box2[2] / 2, box2[0] + box2[2] / 2
    b2_y1, b2_y2 = box2[1] - box2[3] / 2, box2[1] + box2[3] / 2
    inter = (torch.min(b1_x2, b2_x2) - torch.max(b1_x1, b2_x1)).clamp(0) * \
            (torch.min(b1_y2, b2_y2) - torch.max(b1_y1, b2_y1)).clamp(0)
    if aux is not None:
        aux["inter"] = inter.detach()
    w1, h1 = b1_x2 - b1_x1, b1_y2 - b1_y1
    w2, h2 = b2_x2 - b2_x1, b2_y2 - b2_y1
    union = (w1 * h1 + 1e-16) + w2 * h2 - inter                 # :116
    iou = inter / union
    if kind == "iou":
        return iou
    cw = torch.max(b1_x2, b2_x2) - torch.min(b1_x1, b2_x1)
    ch = torch.max(b1_y2, b2_y2) - torch.min(b1_y1, b2_y1)
    if kind == "giou":                                          # :122-124
        c_area = cw * ch + 1e-16
        return iou - (c_area - union) / c_area
    c2 = cw ** 2 + ch ** 2 + 1e-16                              # :127
    rho2 = ((b2_x1 + b2_x2) - (b1_x1 + b1_x2)) ** 2 / 4 + ((b2_y1 + b2_y2) - (b1_y1 + b1_y2)) ** 2 / 4
    if kind == "diou":
        return iou - rho2 / c2
    v = (4 / math.pi ** 2) * torch.pow(torch.atan(w2 / h2) - torch.atan(w1 / h1), 2)   # :133
    if detach_alpha:
        with torch.no_grad():
            alpha = v / (1 - iou + v)                           # :135
    else:
        alpha = v / (1 - iou + v)
    return iou - (rho2 / c2 + v * alpha)


def build_targets(pred_shapes, targets, anchor_vecs, iou_t, pairs=None):
    """utils.py:296-384.  pred_shapes: list of (B,na,ny,nx,no); targets [nt,6] =
    (image, class, xc, yc, w, h) normalised; anchor_vecs: list of [na,2] (anchors / stride).
    Returns per head: tcls, tbox, (b, a, gj, gi), anchors  -- indices are int64.
    pairs: a list that receives, per head, the position a * nt + t of every match among the na * nt (anchor, target) pairs."""
    nt = targets.shape[0]
    tcls, tbox, indices, anch = [], [], [], []
    gain = torch.ones(6)
    for i, shape in enumerate(pred_shapes):
        anchors = anchor_vecs[i]
        gain[2:] = torch.tensor(shape)[[3, 2, 3, 2]].float()    # :328  (nx, ny, nx, ny)
        na = anchors.shape[0]
        at = torch.arange(na).view(na, 1).repeat(1, nt)         # :336
        a, t = [], targets * gain
        if nt:
            j = wh_iou(anchors, t[:, 4:6]) > iou_t              # :352  [na, nt]
            a, t = at[j], t.repeat(na, 1, 1)[j]                 # :361  anchor-major, then target order
            if pairs is not None:
                pairs.append(j.flatten().nonzero().flatten())
        elif pairs is not None:
            pairs.append(torch.zeros(0, dtype=torch.long))
        b, c = t[:, :2].long().t()                              # :367
        gxy = t[:, 2:4]
        gwh = t[:, 4:6]
        gij = gxy.long()                                        # :370 truncation, no clamp
        gi, gj = gij.t()
        indices.append((b, a, gj, gi))
        tbox.append(torch.cat((gxy - gij, gwh), 1))
        anch.append(anchors[a])
        tcls.append(c)
    return tcls, tbox, indices, anch


def compute_loss(p, targets, anchor_vecs, hyp, nc, gr, v4, tobj_out=None):
    """utils.py:209-293.  p: list of [B,na,ny,nx,5+nc] raw logits (fp32).  hyp needs box/obj/cls,
    cls_pw, obj_pw, iou_t, fl_gamma (> 0: both BCE terms become focal, :236-238) and selects CIoU by the presence of
    key 'ciou' (:264).  Returns dict of three [1] tensors.  tobj_out: a list that receives the objectness target of every head
    (what index_put_ leaves at :271)."""
    lcls, lbox, lobj = torch.zeros(1), torch.zeros(1), torch.zeros(1)
    tcls, tbox, indices, anchors = build_targets([tuple(pi.shape) for pi in p], targets, anchor_vecs, hyp["iou_t"])
    cls_pw = torch.tensor([hyp["cls_pw"]])
    obj_pw = torch.tensor([hyp["obj_pw"]])
    gamma = float(hyp.get("fl_gamma", 0.0))

    def bce(pred, true, pw):
        """BCEWithLogitsLoss(pos_weight, 'mean') (:229-230); with fl_gamma > 0 wrapped as FocalLoss(.., gamma) does
        (:184-197, alpha at its default 0.25 of :176): element loss * alpha_factor * (1 - p_t) ** gamma, then the mean"""
        if gamma <= 0:
            return F.binary_cross_entropy_with_logits(pred, true, pos_weight=pw)
        el = F.binary_cross_entropy_with_logits(pred, true, pos_weight=pw, reduction="none")
        prob = torch.sigmoid(pred)                                            # :190
        p_t = true * prob + (1 - true) * (1 - prob)                           # :191
        el = el * (true * 0.25 + (1 - true) * 0.75) * (1.0 - p_t) ** gamma    # :192-194
        return el.mean()                                                      # :196-197
    for i, pi in enumerate(p):
        b, a, gj, gi = indices[i]
        tobj = torch.zeros_like(pi[..., 0])
        nb = b.shape[0]
        if nb:
            ps = pi[b, a, gj, gi]                               # :248
            if v4:                                              # :258-259
                pxy = ps[:, :2].sigmoid() * 2. - 0.5
                pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anchors[i]
            else:                                               # :261-262
                pxy = ps[:, :2].sigmoid()
                pwh = ps[:, 2:4].exp().clamp(max=1E3) * anchors[i]
            pbox = torch.cat((pxy, pwh), 1)
            iou = bbox_iou_xywh(pbox.t(), tbox[i], "ciou" if "ciou" in hyp else "giou")
            lbox = lbox + (1.0 - iou).mean()                    # :268
            tobj[b, a, gj, gi] = (1.0 - gr) + gr * iou.detach().clamp(0).type(tobj.dtype)   # :271
            if nc > 1:                                          # :274-277
                t = torch.full_like(ps[:, 5:], 0.0)
                t[range(nb), tcls[i]] = 1.0
                lcls = lcls + bce(ps[:, 5:], t, cls_pw)           # :277
        lobj = lobj + bce(pi[..., 4], tobj, obj_pw)             # :283
        if tobj_out is not None:
            tobj_out.append(tobj)
    return {"box_loss": lbox * hyp["box"], "obj_loss": lobj * hyp["obj"], "class_loss": lcls * hyp["cls"]}


# ------------------------------------------------------------------------------------------ fp64 reference, per element
MISTAKES = ("first_match_wins", "n_all_matches", "pos_weight_factor", "alpha_not_detached", "tobj_no_clamp",
            "v3_clamp_keeps_gradient", "cls_mean_over_n", "obj_mean_other_head")


def loss_reference(p, targets, anchor_vecs, hyp, nc, gr, v4, dtype=torch.float64, mistake=None):
    """compute_loss (utils.py:209-293) and its gradient with everything behind the match lists evaluated in `dtype`.

    The match lists are those of the fp32 build_targets above (index arithmetic is fp32 by contract).  A match whose image or
    cell index lies outside the prediction tensor -- the reference raises IndexError there -- takes no part and does not count
    in the 1/n of the box and class means: the contract of dyk_yolo_loss, which raises a flag instead.  The objectness target is
    written by an explicit loop in match order, the last match of a cell wins (what index_put_ does on the CPU, :271).

    Returns a dict: box_loss / obj_loss / class_loss (0-dim, dtype), grads (per head: d(sum of the three) / d logits), tobj (per
    head), matches = (tcls, tbox, indices, anch), valid (per head: in-range mask over the matches), pairs (per head: position of
    every match among the na * nt pairs), iou / inter (per head, over the in-range matches).
    mistake: one of MISTAKES, a deliberate error for tests/test_loss_reference.py."""
    assert mistake is None or mistake in MISTAKES, mistake
    pairs = []
    tcls, tbox, indices, anchors = build_targets([tuple(pi.shape) for pi in p], targets, anchor_vecs, hyp["iou_t"], pairs)
    ps_all = [pi.detach().to(dtype).requires_grad_(True) for pi in p]
    lcls, lbox, lobj = torch.zeros(1, dtype=dtype), torch.zeros(1, dtype=dtype), torch.zeros(1, dtype=dtype)
    cls_pw = torch.tensor([hyp["cls_pw"]], dtype=dtype)
    obj_pw = torch.tensor([hyp["obj_pw"]], dtype=dtype)
    gamma = float(hyp.get("fl_gamma", 0.0))

    def bce(pred, true, pw):
        if mistake == "pos_weight_factor":
            el = F.binary_cross_entropy_with_logits(pred, true, reduction="none") * pw
        elif gamma <= 0:
            return F.binary_cross_entropy_with_logits(pred, true, pos_weight=pw)
        else:
            el = F.binary_cross_entropy_with_logits(pred, true, pos_weight=pw, reduction="none")
        if gamma > 0:
            prob = torch.sigmoid(pred)
            p_t = true * prob + (1 - true) * (1 - prob)
            el = el * (true * 0.25 + (1 - true) * 0.75) * (1.0 - p_t) ** gamma
        return el.mean()
    tobjs, valids, ious, inters = [], [], [], []
    for i, pi in enumerate(ps_all):
        B, _, ny, nx, _ = pi.shape
        b, a, gj, gi = (torch.as_tensor(x, dtype=torch.long) for x in indices[i])     # (nt = 0: `a` is an empty list)
        ok = (b >= 0) & (b < B) & (gj >= 0) & (gj < ny) & (gi >= 0) & (gi < nx)
        valids.append(ok)
        n_all = b.shape[0]
        b, a, gj, gi = b[ok], a[ok], gj[ok], gi[ok]
        tobj = torch.zeros(pi.shape[:4], dtype=dtype)
        nb = b.shape[0]
        iou_d, aux = torch.zeros(0, dtype=dtype), {"inter": torch.zeros(0, dtype=dtype)}
        if nb:
            anc = anchors[i][ok].to(dtype)
            ps = pi[b, a, gj, gi]
            if v4:
                pxy = ps[:, :2].sigmoid() * 2. - 0.5
                pwh = (ps[:, 2:4].sigmoid() * 2) ** 2 * anc
            else:
                pxy = ps[:, :2].sigmoid()
                e = ps[:, 2:4].exp().clamp(max=1E3)
                if mistake == "v3_clamp_keeps_gradient":          # d/dt of the clamped value taken as the value itself
                    e = e.detach() * (1.0 + ps[:, 2:4] - ps[:, 2:4].detach())
                pwh = e * anc
            pbox = torch.cat((pxy, pwh), 1)
            iou = bbox_iou_xywh(pbox.t(), tbox[i][ok].to(dtype), "ciou" if "ciou" in hyp else "giou",
                                detach_alpha=mistake != "alpha_not_detached", aux=aux)
            term = (1.0 - iou).mean()
            if mistake == "n_all_matches":
                term = term * (nb / n_all)
            lbox = lbox + term
            iou_d = iou.detach()
            tv = (1.0 - gr) + gr * (iou_d if mistake == "tobj_no_clamp" else iou_d.clamp(0))
            flat = tobj.view(-1)
            cells = (((b * pi.shape[1] + a) * ny + gj) * nx + gi).tolist()
            seen = set()
            for m, c in enumerate(cells):                       # match order; the last one stays
                if mistake == "first_match_wins" and c in seen:
                    continue
                seen.add(c)
                flat[c] = tv[m]
            if nc > 1:
                t = torch.full_like(ps[:, 5:], 0.0)
                t[range(nb), tcls[i][ok]] = 1.0
                term = bce(ps[:, 5:], t, cls_pw)
                if mistake == "n_all_matches":
                    term = term * (nb / n_all)
                if mistake == "cls_mean_over_n":
                    term = term * nc
                lcls = lcls + term
        term = bce(pi[..., 4], tobj, obj_pw)
        if mistake == "obj_mean_other_head":
            term = term * (tobj.numel() / ps_all[(i + 1) % len(ps_all)][..., 0].numel())
        lobj = lobj + term
        tobjs.append(tobj)
        ious.append(iou_d)
        inters.append(aux["inter"])
    out = {"box_loss": lbox * hyp["box"], "obj_loss": lobj * hyp["obj"], "class_loss": lcls * hyp["cls"]}
    (out["box_loss"] + out["obj_loss"] + out["class_loss"]).sum().backward()
    out = {k: v.detach()[0] for k, v in out.items()}
    out.update(grads=[pi.grad for pi in ps_all], tobj=tobjs, matches=(tcls, tbox, indices, anchors), valid=valids, pairs=pairs,
               iou=ious, inter=inters)
    return out


# ------------------------------------------------------------------------------------------ bound of the per-element tests
LOSS_K = 8                    # the kernel may be this many times as far from fp64 as the fp32 evaluation of the reference is
LOSS_FLOOR = 4 * 2.0 ** -23   # ... or this close in any case (relative to the largest / the RMS element of the group)


def channel_groups(no):
    """box 0..3, objectness 4, classes 5.. (absent for nc = 1)"""
    g = {"box": slice(0, 4), "obj": slice(4, 5)}
    if no > 5:
        g["cls"] = slice(5, no)
    return g


def group_errors(got, ref):
    """(max |got - ref| / max |ref|, rms(got - ref) / rms(ref)) in float64; (0, 0) for an all-zero ref matched exactly,
    (inf, inf) for an all-zero ref that is missed"""
    got, ref = got.detach().double().flatten(), ref.detach().double().flatten()
    d = got - ref
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top == 0.0:
        return (0.0, 0.0) if not bool(d.any()) else (math.inf, math.inf)
    return float(d.abs().max()) / top, float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def loss_errors(got, ref):
    """got / ref: results in the layout of loss_reference (grads, tobj, the three scalars).  -> {name: (max-normalised,
    rms-normalised)} for tobj and every channel group of every head, {name: (relative, relative)} for the scalars"""
    out = {}
    for h, (g, r) in enumerate(zip(got["grads"], ref["grads"])):
        for name, sl in channel_groups(r.shape[-1]).items():
            out["head%d.%s" % (h, name)] = group_errors(g[..., sl], r[..., sl])
        out["head%d.tobj" % h] = group_errors(got["tobj"][h], ref["tobj"][h])
    for k in ("box_loss", "obj_loss", "class_loss"):
        out[k] = group_errors(torch.as_tensor(got[k]).reshape(1), torch.as_tensor(ref[k]).reshape(1))
    return out


def loss_bound(yard):
    """the largest error allowed per entry of loss_errors, from the errors `yard` of the reference evaluated in fp32"""
    return {k: tuple(max(LOSS_K * e, LOSS_FLOOR) for e in v) for k, v in yard.items()}


# ------------------------------------------------------------------------------------------ input families
V3_CFG, V4_CFG = "kaist_yolov3.cfg", "kaist_dyolov4_fshare_global_concat_se3.cfg"
# seed % 6 selects the configuration of a family: parameterisation / IoU kind, classes, gr, positive weights, focal gamma
LOSS_CONFIGS = (
    dict(cfg=V4_CFG, nc=1, gr=1.0, obj_pw=1.0, cls_pw=1.0, fl_gamma=0.0),
    dict(cfg=V3_CFG, nc=2, gr=0.5, obj_pw=1.7, cls_pw=0.6, fl_gamma=0.0),
    dict(cfg=V4_CFG, nc=3, gr=0.0, obj_pw=1.7, cls_pw=0.6, fl_gamma=1.5),
    dict(cfg=V3_CFG, nc=1, gr=1.0, obj_pw=1.7, cls_pw=0.6, fl_gamma=1.5),
    dict(cfg=V4_CFG, nc=2, gr=1.0, obj_pw=1.7, cls_pw=0.6, fl_gamma=0.0),
    dict(cfg=V3_CFG, nc=3, gr=0.5, obj_pw=1.0, cls_pw=1.0, fl_gamma=0.0),
)
CHUNK_NT = (85, 86, 171)      # na * nt = 255, 258, 513: one short of a 256-pair chunk, just over one, just over two
FAMILY_H, FAMILY_W = 128, 160
LOSS_KINDS = ("chunk_edges", "crowded", "huge", "dup_chain", "saturated", "disjoint", "outside")
# (kind, seed) of every case the tests run; `huge` (quadratic last-match scan) for one configuration only
LOSS_FAMILIES = (
    ("chunk_edges", 0), ("chunk_edges", 7), ("chunk_edges", 14), ("chunk_edges", 3), ("chunk_edges", 10), ("chunk_edges", 17),
    ("crowded", 1), ("crowded", 2), ("crowded", 10),
    ("huge", 0),
    ("dup_chain", 0), ("dup_chain", 5), ("dup_chain", 2),
    ("saturated", 0), ("saturated", 1), ("saturated", 2), ("saturated", 3),
    ("disjoint", 1), ("disjoint", 3), ("disjoint", 5),
    ("outside", 4), ("outside", 1),
)


def _boxes(g, n, B, nc, wlo, whi):
    """n targets: image indices ascending, classes, centres inside the image, widths log-uniform in [wlo, whi] pixels and
    pedestrian aspect ratios (the anchors' are 1.9 .. 2.5)"""
    t = torch.zeros(n, 6)
    t[:, 0] = torch.randint(0, B, (n,), generator=g).float().sort()[0]
    t[:, 1] = torch.randint(0, nc, (n,), generator=g).float()
    t[:, 2:4] = torch.rand(n, 2, generator=g) * 0.9 + 0.05
    w = wlo * (whi / wlo) ** torch.rand(n, generator=g)
    t[:, 4] = w / FAMILY_W
    t[:, 5] = w * (1.9 + 0.8 * torch.rand(n, generator=g)) / FAMILY_H
    return t


def loss_input_family(kind, seed):
    """Deterministic inputs of the loss kernels -> (cfg, nc, hyp overrides, gr, logits per head, targets [nt,6]).
    B = 4 (huge: 2) at 128 x 160: heads of 16x20, 8x10, 4x5 cells (v4 order; v3 has them reversed).  seed % 6 selects
    LOSS_CONFIGS; logits are randn * 1.5 unless the kind says otherwise.
      chunk_edges  nt = CHUNK_NT[seed // 6 % 3]: the 256-pair chunks of the ordered compaction end inside / at the list
      crowded      nt = 200 of every size the anchors cover: > 256 matches per head, the strided match loops
      huge         B = 2, nt = 2000 sized for the finest head: > 4096 matches there (the scan without the LDS keys)
      dup_chain    nt = 900: groups of 3 and 4 targets in one cell with the same anchors, 265 targets apart (members of a group
                   lie in different 256-pair chunks), targets exactly on cell borders of every head, crowded fillers
      saturated    a quarter of the objectness / class logits moved to +-[55, 65], a quarter of the xy logits * 13 (about +-20);
                   wh logits uniform in [-12, 12] (v3: exp(t) >= 1e3 from t = 6.9) or [-3, 20] (v4).  The ranges are as wide
                   as fp32 itself allows: below -3 the v4 box height (y + h/2) - (y - h/2) loses enough bits that the fp32
                   reference leaves the 1e-6 conditioning cap (from about -7 it is 0 and atan(w1 / h1) NaN), and with the focal
                   term a logit between 8 and 17 meets 1 - sigmoid(x) at 1 to 4 bits (error x * gamma * 2^-24 of the largest
                   gradient), so the saturated logits skip that band
      disjoint     narrow targets at the left edge of their cells, x logits in [3, 5] (predicted centre at the right edge) and
                   wh logits in [-3, -1]: no intersection, negative GIoU (v3 / GIoU configurations only)
      outside      crowded, plus targets with x == 1.0 or y == 1.0: their cell index is nx / ny, the flag must be raised and
                   they must not count in the means"""
    c = LOSS_CONFIGS[seed % 6]
    cfg, nc, v4 = c["cfg"], c["nc"], c["cfg"] == V4_CFG
    g = torch.Generator().manual_seed(1000 * (1 + LOSS_KINDS.index(kind)) + seed)
    B = 2 if kind == "huge" else 4
    strides = (8, 16, 32) if v4 else (32, 16, 8)
    shapes = [(B, 3, FAMILY_H // s, FAMILY_W // s, 5 + nc) for s in strides]
    p = [torch.randn(s, generator=g) * 1.5 for s in shapes]
    if kind == "chunk_edges":
        t = _boxes(g, CHUNK_NT[seed // 6 % 3], B, nc, 12.0, 70.0)
        t[-1, 4], t[-1, 5] = 30.0 / FAMILY_W, 70.0 / FAMILY_H      # matches the last anchor of every head: the last pair is a match
    elif kind == "crowded":
        t = _boxes(g, 200, B, nc, 12.0, 70.0)
    elif kind == "huge":
        assert v4
        t = _boxes(g, 2000, B, nc, 15.0, 23.0)
    elif kind == "dup_chain":
        t = _boxes(g, 900, B, nc, 12.0, 70.0)
        # a group shares its cell on every head (the coarsest cells are 32 px) and its size, so it matches the same anchors
        for q, (first, members, x, y, w) in enumerate([(5, 4, 0.3031, 0.2721, 20.0), (9, 3, 0.7106, 0.6412, 40.0),
                                                       (50, 3, 0.5201, 0.8102, 17.0)]):
            for k in range(members):
                r = first + 265 * k
                t[r, 0] = q % B
                t[r, 2], t[r, 3] = x + 1e-4 * k, y + 1e-4 * k
                t[r, 4], t[r, 5] = (w + 0.3 * k) / FAMILY_W, (2.2 * w + 0.5 * k) / FAMILY_H
        for k, r in enumerate(range(100, 112)):                  # centres exactly on the cell borders of the three grids
            t[r, 2] = (3 + k) / 20.0 if k % 3 == 0 else ((2 + k // 2) / 10.0 if k % 3 == 1 else (1 + k // 4) / 5.0)
            t[r, 3] = (2 + k) / 16.0 if k % 3 == 0 else ((1 + k // 2) / 8.0 if k % 3 == 1 else (1 + k // 6) / 4.0)
    elif kind == "saturated":
        t = _boxes(g, 120, B, nc, 12.0, 70.0)
        for pi in p:
            hot = torch.rand(pi[..., 4:].shape, generator=g) < 0.25
            big = torch.sign(pi[..., 4:]) * (55.0 + 10.0 * torch.rand(pi[..., 4:].shape, generator=g))
            pi[..., 4:] = torch.where(hot, big, pi[..., 4:])
            hot = torch.rand(pi[..., :2].shape, generator=g) < 0.25
            pi[..., :2] = torch.where(hot, pi[..., :2] * 13.0, pi[..., :2])
            lo, hi = (-3.0, 20.0) if v4 else (-12.0, 12.0)
            pi[..., 2:4] = lo + (hi - lo) * torch.rand(pi[..., 2:4].shape, generator=g)
    elif kind == "disjoint":
        assert not v4
        t = _boxes(g, 90, B, nc, 8.0, 9.0)
        t[:, 5] = (33.0 + 60.0 * torch.rand(90, generator=g)) / FAMILY_H
        t[:, 2] = (torch.randint(1, 19, (90,), generator=g).float() + 0.05 + 0.1 * torch.rand(90, generator=g)) / 20.0
        for pi in p:
            pi[..., 0] = 3.0 + 2.0 * torch.rand(pi[..., 0].shape, generator=g)
            pi[..., 2:4] = -3.0 + 2.0 * torch.rand(pi[..., 2:4].shape, generator=g)
    elif kind == "outside":
        t = _boxes(g, 120, B, nc, 12.0, 70.0)
        t[7, 2], t[41, 3], t[88, 2], t[88, 3] = 1.0, 1.0, 1.0, 1.0
    else:
        raise ValueError(kind)
    over = dict(obj_pw=c["obj_pw"], cls_pw=c["cls_pw"], fl_gamma=c["fl_gamma"])
    return cfg, nc, over, c["gr"], p, t
