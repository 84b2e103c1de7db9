"""Case matrix of the row-wise multi-label NMS (dyk_nms_rows), shared by tests/test_nms_rows.py (CPU) and
tests/test_gpu_nms_rows.py (GPU).  Inputs come from tests/golden/cases.py `nms_pred`, which takes any class count.

Alive rows / candidates per image of the matrix (seed 77, B = 3), measured on the CPU with `candidate_counts` below; the tests
recompute them and assert only the relation they rely on (fits / overflows):
  s80      N 1500 nc  80 conf 0.6   131/3955  133/4005  128/4099
  s80_cap  N 1500 nc  80 conf 0.7    99/2055   93/2177   96/2318
  s33      N 2100 nc  33 conf 0.45  186/3580  159/2904  185/3565
  s20      N 1100 nc  20 conf 0.5   168/1872  150/1420  170/1904
  s365     N  700 nc 365 conf 0.55  136/21056 156/26716 164/27143
  ties3    N  600 nc   3 conf 0.1   305/915   316/948   290/870
"""
import sys

import torch

from helpers import GOLDEN

sys.path.insert(0, GOLDEN)
import cases  # noqa: E402

IOU, MAX_NUM, SEED, B = 0.6, 100, 77, 3

MATRIX = {
    "s80": dict(N=1500, nc=80, kind="sparse", conf=0.6),
    "s80_cap": dict(N=1500, nc=80, kind="sparse", conf=0.7),
    "s33": dict(N=2100, nc=33, kind="sparse", conf=0.45),
    "s20": dict(N=1100, nc=20, kind="sparse", conf=0.5),
    "s365": dict(N=700, nc=365, kind="sparse", conf=0.55),
    "ties3": dict(N=600, nc=3, kind="ties", conf=0.1),
}

S80_CLASSES = [0, 3, 7, 11, 19, 23, 31, 40, 41, 42, 55, 63, 64, 65, 78, 79]      # 16 indices, both 64-class chunks

_preds = {}


def pred(name):
    """[B, N, 5 + nc] fp32 on the host; built once per name, never modified by the tests"""
    if name not in _preds:
        c = MATRIX[name]
        _preds[name] = cases.nms_pred(dict(name=name, B=B, N=c["N"], nc=c["nc"], kind=c["kind"], seed=SEED))
    return _preds[name]


def candidate_counts(p, conf, classes=None):
    """(alive rows, candidates) per image as reference build_utils/utils.py:408-409, :416, :423, :430-431 define them: fp32
    products, strict comparisons"""
    alive = (p[..., 4] > conf) & ((p[..., 2:4] > 2) & (p[..., 2:4] < 4096)).all(-1)
    ok = ((p[..., 5:] * p[..., 4:5]) > conf) & alive[..., None]
    if classes:
        sel = torch.zeros(p.shape[2] - 5, dtype=torch.bool)
        sel[list(classes)] = True
        ok = ok & sel
    return alive.sum(1).tolist(), ok.sum((1, 2)).tolist()


def dense_pred(nb, N, nc, seed):
    """every row alive (obj in [0.9, 1), boxes well inside 2 < w,h < 4096), class scores uniform in [0, 1): with
    conf_thres = DENSE_CONF about half of the classes of every row pass.  Boxes cluster so that suppression has work."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(nb, N, 5 + nc)
    p[..., 0] = torch.rand(nb, N, generator=g) * 300 + 40
    p[..., 1] = torch.rand(nb, N, generator=g) * 200 + 40
    p[..., 2] = torch.rand(nb, N, generator=g) * 60 + 16
    p[..., 3] = torch.rand(nb, N, generator=g) * 120 + 32
    p[..., 4] = torch.rand(nb, N, generator=g) * 0.1 + 0.9
    p[..., 5:] = torch.rand(nb, N, nc, generator=g)
    return p


DENSE_CONF = 0.475
EDGE_N = [1, 63, 64, 65, 1023, 1025]
EDGE_NC = [2, 63, 64, 65, 129]
EDGE_ORACLE = [(n, c) for n in (63, 64, 65) for c in (64, 65)]


def special_pred():
    """[3, 96, 8] (nc = 3), conf_thres = SPECIAL_CONF = 0.25.  Image 0: ordinary rows with one special value each; image 1: no
    alive row; image 2: alive rows, no passing class.  Returns (pred, what) with `what` naming the special rows of image 0."""
    g = torch.Generator().manual_seed(5)
    p = torch.zeros(3, 96, 8)
    p[..., 0] = torch.rand(3, 96, generator=g) * 200 + 60
    p[..., 1] = torch.rand(3, 96, generator=g) * 200 + 60
    p[..., 2] = torch.rand(3, 96, generator=g) * 40 + 16
    p[..., 3] = torch.rand(3, 96, generator=g) * 80 + 32
    p[..., 4] = torch.rand(3, 96, generator=g) * 0.4 + 0.6
    p[..., 5:] = torch.rand(3, 96, 3, generator=g) * 0.5 + 0.5
    nan, inf = float("nan"), float("inf")
    what = {}
    r = iter(range(2, 96, 3))

    def put(name, col, val):
        i = next(r)
        p[0, i, col] = val
        what[name] = i

    for name, val in (("obj_nan", nan), ("obj_inf", inf), ("obj_neg0", -0.0), ("obj_eq_thres", 0.25)):
        put(name, 4, val)
    for name, val in (("cls_nan", nan), ("cls_inf", inf), ("cls_neg0", -0.0)):
        put(name, 6, val)
    for col, tag in ((2, "w"), (3, "h")):
        for name, val in (("nan", nan), ("inf", inf), ("neg0", -0.0), ("eq2", 2.0), ("eq4096", 4096.0)):
            put("%s_%s" % (tag, name), col, val)
    i = next(r)                                    # conf = 0.5 * 0.5 = 0.25 exactly: not > conf_thres (the others: 0.1, 0.125)
    p[0, i, 4], p[0, i, 5:] = 0.5, torch.tensor([0.5, 0.2, 0.25])
    what["conf_eq_thres"] = i
    p[1, :, 4] = 0.1                               # image 1: no alive row
    p[2, :, 4] = 0.5                               # image 2: every row alive, every conf = 0.5 * 0.3 = 0.15 < conf_thres
    p[2, :, 5:] = 0.3
    return p, what


SPECIAL_CONF = 0.25
