"""Shared test helpers (fixture loading, oracle construction)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CFGS = ["kaist_yolov3", "kaist_dyolov3_add_sl", "kaist_dyolov4_fshare_global_concat_se3",
        "kaist_dyolov4_mobilenetv3_fshare_global_cse3", "kaist_dyolov4_mobilenetv2_fshare_global_cse3",
        "kaist_dyolov3_concat_inc"]
C1, C2, C3, C5, MNV2, INC = CFGS

# Trajectory bound of the fused optimizers (tests/test_gpu_optim.py, "twelve steps against torch.optim"): the kernel's distance to
# torch.optim in fp64 may be at most K times torch.optim-fp32's own.  K = twice the largest ratio measured on MI355X, rounded up to
# one digit, never above 4; the twelve measured ratios stand in the docstrings of the two trajectory tests (largest: 1.00 for both).
OPTIM_K = {"adam": 2, "sgd": 2}


def golden_sections(name):
    from build_utils.parse_config import sections_from_json
    return sections_from_json(os.path.join(GOLDEN, "parse_%s.json" % name))


def same_sections(a, b):
    """exact equality of two parsed cfgs, including value types"""
    if len(a) != len(b):
        return False
    for da, db in zip(a, b):
        if list(da.keys()) != list(db.keys()):
            return False
        for k in da:
            va, vb = da[k], db[k]
            if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
                if not (isinstance(va, np.ndarray) and isinstance(vb, np.ndarray)):
                    return False
                if va.dtype != vb.dtype or va.shape != vb.shape or not np.array_equal(va, vb):
                    return False
            elif type(va) is not type(vb) or va != vb:
                return False
    return True


def oracle_net(name):
    from oracle.model import OracleNet
    return OracleNet(golden_sections(name), "config/%s.cfg" % name)


def hyp(name="hyp.scratch.4"):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def tref_to_nchw(plan, t):
    """a plan tensor (dyk.plan.TRef: channels-last rows of `ld` elements inside an arena) as a float32 NCHW CPU tensor"""
    import torch
    es = t.esize
    dt = torch.float32 if es == 4 else torch.bfloat16
    a = plan.arenas[t.arena].tensor
    n = t.npix * t.ld
    flat = a[t.off:t.off + (n - (t.ld - t.C)) * es].view(dt)
    v = torch.as_strided(flat, (t.B, t.H, t.W, t.C), (t.H * t.W * t.ld, t.W * t.ld, t.ld, 1))
    return v.float().permute(0, 3, 1, 2).contiguous().cpu()


_LOSS_FAMILY_CACHE = {}


def loss_family(kind, seed):
    """oracle.loss.loss_input_family(kind, seed) with everything a loss test needs, computed once per process and shared (do not
    modify): dict(cfg, nc, hyp, gr, v4, p, targets, anchor_vecs, r64, r32) -- r64 / r32 = oracle.loss.loss_reference in float64 /
    float32, the reference and the yardstick of tests/test_loss_reference.py and tests/test_gpu_loss_elements.py"""
    import sys
    import torch
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import cases
    from oracle import loss as oloss
    key = (kind, seed)
    if key not in _LOSS_FAMILY_CACHE:
        cfg, nc, over, gr, p, targets = oloss.loss_input_family(kind, seed)
        anchors, strides, v4 = cases.head_geometry(cfg)
        av = [torch.tensor(a, dtype=torch.float32) / s for a, s in zip(anchors, strides)]
        hyp = dict(cases.load_hyp("hyp.scratch.4" if v4 else "hyp.scratch"), **over)
        f = dict(cfg=cfg, nc=nc, hyp=hyp, gr=gr, v4=v4, p=p, targets=targets, anchor_vecs=av)
        f["r64"] = oloss.loss_reference(p, targets, av, hyp, nc, gr, v4, dtype=torch.float64)
        f["r32"] = oloss.loss_reference(p, targets, av, hyp, nc, gr, v4, dtype=torch.float32)
        _LOSS_FAMILY_CACHE[key] = f
    return _LOSS_FAMILY_CACHE[key]
