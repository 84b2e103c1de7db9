"""Shared by tests/test_wide_heads.py (host) and tests/test_gpu_wide_heads.py: the class counts at which the detection heads
change layout, the per-case cfg written from the builder-authored template tests/golden/tiny_kaist_wide_heads.cfg (two [yolo]
heads at strides 8 and 16, head-conv input channels 48 and 64), its inputs and targets, and the oracle's results (computed once
per process and shared: do not modify)."""
import os
import re

import torch

from helpers import GOLDEN

TEMPLATE = os.path.join(GOLDEN, "tiny_kaist_wide_heads.cfg")
NA = 3
# nc -> na * no.  5: the last count on the 32-channel rows (same op list as before); 6: first width over the line, 31 pad
# channels; 20: rows of 96, not a power of two; 27: no padding at all; 80: one pad channel
NCS = [5, 6, 20, 27, 80]
WIDE = [nc for nc in NCS if NA * (5 + nc) > 32]
B, H, W = 2, 32, 64


def expected_ld(nc):
    """the width rule, restated: 32 up to 32 channels, above that the next multiple of 32"""
    c = NA * (5 + nc)
    return 32 if c <= 32 else -(-c // 32) * 32


def write_cfg(tmp_dir, nc, v4=False):
    """the template with classes= and the head filters= rewritten for `nc`; the FILE NAME selects the box decode flavour (v4 when
    it contains 'yolov4', reference models.py:124-131).  -> path"""
    text = open(TEMPLATE).read()
    text = re.sub(r"classes=1\b", "classes=%d" % nc, text)
    text = re.sub(r"filters=18\b", "filters=%d" % (NA * (5 + nc)), text)
    assert text.count("classes=%d" % nc) == 2 and text.count("filters=%d\n" % (NA * (5 + nc))) == 2
    path = os.path.join(str(tmp_dir), "tiny_%s_wide_nc%d.cfg" % ("yolov4" if v4 else "v3", nc))
    with open(path, "w") as f:
        f.write(text)
    return path


def inputs():
    g = torch.Generator().manual_seed(4242)
    return torch.rand(B, 3, H, W, generator=g)


def targets(nc):
    """(image, class, xc, yc, w, h): the first and the last class index, on both images; sizes that match anchors of both heads"""
    return torch.tensor([[0, 0, 0.30, 0.40, 0.20, 0.45], [0, nc - 1, 0.70, 0.55, 0.40, 0.60],
                         [1, nc - 1, 0.50, 0.50, 0.25, 0.80], [1, 0, 0.20, 0.30, 0.55, 0.70]], dtype=torch.float32)


def hyp():
    from helpers import hyp as load
    return load("hyp.scratch")


def oracle_backward_from(o, nc, v4, heads):
    """{name: gradient} of the oracle's autograd through the net of oracle() result `o`, seeded with the gradient of the oracle's
    compute_loss evaluated AT the head tensors `heads` (CPU, fp32) instead of at the oracle's own.  The detection loss is only
    piecewise smooth in the box logits (the enclosing-box min / max of GIoU / CIoU, the clamp of the objectness target): moving
    the logits by a bf16 rounding flips branches and moves single elements of its gradient by tens of per cent of the tensor's
    scale, on the reference itself.  Seeding both backward passes with the gradient at the SAME logits keeps the network's
    backward comparable element by element."""
    from oracle import loss as oloss
    net, sd = o["net"], o["sd"]
    at = [t.detach().float().cpu().clone().requires_grad_(True) for t in heads]
    out = oloss.compute_loss(at, targets(nc), net.anchor_vecs(), hyp(), nc, 1.0, v4)
    (out["box_loss"] + out["obj_loss"] + out["class_loss"]).backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    tp = net.forward({k: leaves.get(k, v.clone()) for k, v in sd.items()}, inputs(), training=True)
    torch.autograd.backward(tp, [t.grad for t in at])
    return {k: v.grad for k, v in leaves.items()}


_ORACLE = {}


def oracle(tmp_dir, nc, v4=False):
    """dict(cfg, net, sd, eval_io, eval_p, train_p, loss (three floats), grads {name: tensor}) of the oracle on the case's cfg
    with OracleNet.synth_state(3): forward in both modes, compute_loss on targets(nc) and autograd through both, fp32 on the CPU"""
    key = (nc, v4)
    if key not in _ORACLE:
        from build_utils.parse_config import parse_model_cfg
        from oracle import loss as oloss
        from oracle.model import OracleNet
        cfg = write_cfg(tmp_dir, nc, v4)
        net = OracleNet(parse_model_cfg(cfg), cfg)
        sd = net.synth_state(3)
        x = inputs()
        with torch.no_grad():
            io, p = net.forward({k: v.clone() for k, v in sd.items()}, x, training=False)
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
        sdt = {k: leaves.get(k, v.clone()) for k, v in sd.items()}
        tp = net.forward(sdt, x, training=True)
        out = oloss.compute_loss(tp, targets(nc), net.anchor_vecs(), hyp(), nc, 1.0, v4)
        (out["box_loss"] + out["obj_loss"] + out["class_loss"]).backward()
        _ORACLE[key] = dict(cfg=cfg, net=net, sd=sd, eval_io=io, eval_p=[t for t in p], train_p=[t.detach() for t in tp],
                            loss=[float(out[k]) for k in ("box_loss", "obj_loss", "class_loss")],
                            grads={k: v.grad for k, v in leaves.items()})
    return _ORACLE[key]
