"""The loss kernels of csrc/loss.hip (target assignment, CIoU / GIoU box term, dense objectness BCE, class BCE, their analytic
gradients) per element against oracle.loss.loss_reference in float64, on the input families of oracle.loss.loss_input_family:
several 256-pair chunks of the ordered compaction, strided match loops, more than 4096 matches on a head (the last-match scan
without its LDS keys), chains of duplicates across chunks, positive weights other than 1, focal terms, saturated logits and the v3
clamp, disjoint boxes under GIoU, targets outside the grid.  tests/test_loss_reference.py shows on the CPU that every family takes
its path, that the bound below is tight (fp32 itself is within 1e-6 of fp64 there) and that it catches eight plausible mistakes.

Bound: for tobj and the box / objectness / class gradients of every head, max |got - ref64| / max |ref64| and
rms(got - ref64) / rms(ref64) may be at most LOSS_K = 8 times what the SAME reference evaluated in float32 on the CPU shows, with a
floor of 4 * 2^-23; the three scalars likewise on their relative error.  The factor allows for device expf / log1pf / atanf / powf
of a few ulp where the CPU's are at most 1, and for the atomic sums on shared cells associating differently.

Reproducibility: tobj, the objectness gradients and the scalars are bit-identical between two runs, and so are the box and class
gradients of every cell that has a single match.  Cells shared by several matches are exempt: their gradients are added with
atomicAdd, whose order is not defined.

MEASURED on MI355X, worst error / max(fp32 reference's error, floor / 8) over all entries and cases of a family (bound 8):
    chunk_edges 1.93 (class_loss)   crowded 2.42 (class_loss)   huge 1.41 (head2.obj)   dup_chain 1.61 (obj_loss)
    saturated 2.19 (head2.cls)      disjoint 1.72 (head1.obj)   outside 1.33 (head2.cls)
The gradient groups sit between 0.7 and 2.2: the kernel's forward-mode box gradient and closed-form BCE / focal derivatives round
like autograd in fp32 does.  The scalars' ratios are against the floor (the fp32 reference sums them to 1e-8).
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import loss_family
from oracle import loss as oloss
from test_gpu_loss_nms import _fake_model, cases

pytestmark = pytest.mark.gpu

FAMILIES = list(oloss.LOSS_FAMILIES)
FID = ["%s-%d" % f for f in FAMILIES]
SCALARS = ("box_loss", "obj_loss", "class_loss")
_RUNS = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(kind, seed):
    """two runs of build_utils.utils.compute_loss + backward on the family, as CPU tensors in the layout of loss_reference"""
    key = (kind, seed)
    if key not in _RUNS:
        from build_utils.utils import compute_loss
        f = loss_family(kind, seed)
        runs = []
        for _ in range(2):
            model = _fake_model(f["cfg"], f["nc"], f["hyp"], f["gr"])
            p = [t.cuda().requires_grad_(True) for t in f["p"]]
            out = compute_loss(p, f["targets"].cuda(), model)
            (out["box_loss"] + out["obj_loss"] + out["class_loss"]).backward()
            r = {k: out[k].detach().cpu()[0] for k in SCALARS}
            r["grads"] = [t.grad.cpu() for t in p]
            r["tobj"] = [t.cpu().clone() for t in model._dyk_loss_keep[1]]
            r["flag"] = int(model._dyk_loss_flag.item())
            runs.append(r)
        _RUNS[key] = runs
    return _RUNS[key]


def _cell_counts(f, h):
    """number of in-range matches per cell of head h, [B, na, ny, nx]"""
    r = f["r64"]
    ok = r["valid"][h]
    b, a, gj, gi = [x[ok] for x in r["matches"][2][h]]
    n = torch.zeros(f["p"][h].shape[:4], dtype=torch.long)
    n.index_put_((b, a, gj, gi), torch.ones_like(b), accumulate=True)
    return n


# ------------------------------------------------------------------ target assignment, bit for bit
@pytest.mark.parametrize("cfg", [oloss.V3_CFG, oloss.V4_CFG], ids=["v3", "v4"])
@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_build_targets_bit_exact_on_every_family(kind, seed, cfg):
    from build_utils.utils import build_targets
    f = loss_family(kind, seed)
    tg = f["targets"]
    B = f["p"][0].shape[0]
    model = _fake_model(cfg, f["nc"], f["hyp"], 1.0)
    shapes = cases.head_shapes(cfg, B, oloss.FAMILY_H, oloss.FAMILY_W, 5 + f["nc"])
    av = [m.anchor_vec for m in model.module_list]
    pairs = []
    tcls_r, tbox_r, idx_r, anch_r = oloss.build_targets(shapes, tg, av, f["hyp"]["iou_t"], pairs)
    tcls, tbox, indices, anch = build_targets([torch.zeros(s, device="cuda") for s in shapes], tg.cuda(), model)
    assert max(len(q) for q in pairs) > 0
    for h in range(3):
        assert len(indices[h]) == 4 and all(x.dtype == torch.int64 for x in indices[h])
        assert indices[h][0].shape[0] == idx_r[h][0].shape[0], (h, "counts")
        for k in range(4):
            assert torch.equal(indices[h][k].cpu(), idx_r[h][k]), (h, k)
        assert torch.equal(_bits(tbox[h].cpu()), _bits(tbox_r[h])), h
        assert torch.equal(_bits(anch[h].cpu()), _bits(anch_r[h])), h
        assert tcls[h].dtype == torch.int64 and torch.equal(tcls[h].cpu(), tcls_r[h]), h


# ------------------------------------------------------------------ loss and gradient: structure, exact
@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_structure_of_tobj_and_the_sparse_gradients(kind, seed):
    f = loss_family(kind, seed)
    got = _run(kind, seed)[0]
    assert got["flag"] == (1 if kind == "outside" else 0)
    for k in SCALARS:
        assert bool(torch.isfinite(got[k]))
    for h in range(3):
        n = _cell_counts(f, h)
        g, tobj = got["grads"][h], got["tobj"][h]
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(tobj).all())
        # tobj is written on matched cells only; where the reference's value is not 0 (gr = 1 with a clamped IoU gives 0) it is set
        assert not bool(tobj[n == 0].any()), h
        assert torch.equal(tobj != 0, f["r64"]["tobj"][h] != 0), h
        assert not bool(_bits(g[..., :4])[n == 0].any()), (h, "box gradient off the matched cells")
        assert not bool(_bits(g[..., 5:])[n == 0].any()), (h, "class gradient off the matched cells")
        assert bool((g[..., :4][n > 0] != 0).any())


# ------------------------------------------------------------------ loss and gradient: values
def _ratios(got, f):
    """{entry: (err / max(yardstick, floor / K)) for the max- and the rms-normalised error}: within the bound iff <= LOSS_K"""
    yard = oloss.loss_errors(f["r32"], f["r64"])
    err = oloss.loss_errors(got, f["r64"])
    lo = oloss.LOSS_FLOOR / oloss.LOSS_K
    return {k: tuple(e / max(y, lo) for e, y in zip(err[k], yard[k])) for k in err}, err, yard


@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_values_within_eight_times_the_fp32_reference_error(kind, seed):
    f = loss_family(kind, seed)
    got = _run(kind, seed)[0]
    ratios, err, yard = _ratios(got, f)
    worst = max(ratios, key=lambda k: max(ratios[k]))
    print("%s-%d worst ratio %.2f on %s (err %.2e / %.2e, fp32 reference %.2e / %.2e)"
          % ((kind, seed, max(ratios[worst]), worst) + err[worst] + yard[worst]))
    print("    per entry:", {k: "%.2f" % max(v) for k, v in ratios.items()})
    bound = oloss.loss_bound(yard)
    for k in err:
        assert err[k][0] <= bound[k][0] and err[k][1] <= bound[k][1], (k, err[k], bound[k], yard[k])


# ------------------------------------------------------------------ two runs
@pytest.mark.parametrize("kind,seed", FAMILIES, ids=FID)
def test_two_runs_agree_bit_for_bit_outside_shared_cells(kind, seed):
    f = loss_family(kind, seed)
    a, b = _run(kind, seed)
    for k in SCALARS:
        assert torch.equal(_bits(a[k].reshape(1)), _bits(b[k].reshape(1))), k
    for h in range(3):
        single = _cell_counts(f, h) <= 1
        assert torch.equal(_bits(a["tobj"][h]), _bits(b["tobj"][h])), h
        assert torch.equal(_bits(a["grads"][h][..., 4]), _bits(b["grads"][h][..., 4])), h
        assert torch.equal(_bits(a["grads"][h])[single], _bits(b["grads"][h])[single]), h
        assert int(single.sum()) > 0 or kind == "huge"


# ------------------------------------------------------------------ the C ABI: three buffer layouts, guard bands
GUARD = 64                      # 32-bit words on either side of every buffer (keeps 8-byte alignment)
GUARD_BITS = 0x7fa5a5a5         # a NaN when read as fp32
FILL_BITS = 0x7fc12345          # what every buffer holds before the call: NaN as fp32 / fp64, huge as an integer


class Guarded:
    """`words` 32-bit words pre-filled with NaN bits between two guard bands, in one device allocation"""

    def __init__(self, words):
        self.words = words
        self.full = torch.full((words + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
        self.body = self.full[GUARD:GUARD + words]
        self.body.fill_(FILL_BITS)

    def ptr(self, word=0):
        return self.body.data_ptr() + 4 * word

    def intact(self):
        return bool((self.full[:GUARD] == GUARD_BITS).all()) and bool((self.full[GUARD + self.words:] == GUARD_BITS).all())


def _abi_call(f, layout):
    """dyk_yolo_loss with hand-built descriptors -> dict(out, dp, tobj, flag, counts, bufs)"""
    from dyk import lib as L
    p = [t.cuda().contiguous() for t in f["p"]]
    tg = f["targets"].cuda().contiguous()
    nt, na, no = tg.shape[0], 3, 5 + f["nc"]
    cap = na * nt
    n_dp = [t.numel() for t in p]
    n_to = [t.numel() // no for t in p]
    bufs = {}
    t = L.DykTargetsDesc()
    t.targets, t.nt, t.nheads, t.na, t.iou_t = tg.data_ptr(), nt, 3, na, float(f["hyp"]["iou_t"])
    for h in range(3):
        t.ny[h], t.nx[h] = p[h].shape[2], p[h].shape[3]
        for q, v in enumerate(f["anchor_vecs"][h].reshape(-1).tolist()):
            t.anchor_vec[h][q] = v
    for name, words in (("counts", 3), ("indices", 2 * 3 * 4 * cap), ("tbox", 3 * cap * 4), ("anch", 3 * cap * 2),
                        ("tcls", 2 * 3 * cap), ("out", 3)):
        bufs[name] = Guarded(words)
    t.counts, t.indices, t.tbox = bufs["counts"].ptr(), bufs["indices"].ptr(), bufs["tbox"].ptr()
    t.anch, t.tcls = bufs["anch"].ptr(), bufs["tcls"].ptr()
    d = L.DykLossDesc()
    d.nheads, d.B, d.no, d.nc = 3, p[0].shape[0], no, f["nc"]
    d.v4, d.ciou = int(f["v4"]), int("ciou" in f["hyp"])
    hyp = f["hyp"]
    d.hyp_box, d.hyp_obj, d.hyp_cls = hyp["box"], hyp["obj"], hyp["cls"]
    d.cls_pw, d.obj_pw, d.gr = hyp["cls_pw"], hyp["obj_pw"], f["gr"]
    d.fl_gamma, d.fl_alpha = hyp["fl_gamma"], 0.25
    d.out = bufs["out"].ptr()
    body = sum(n_dp) + sum(n_to)
    assert body % 2 == 0                                       # the trailing acc of the tail layout stays 8-byte aligned
    if layout in ("head", "tail"):
        bufs["flat"] = flat = Guarded(body + 26 if layout == "head" else body + 25)
        off = 26 if layout == "head" else 0
        dp_at, to_at = [], []
        for n in n_dp:
            dp_at.append(off)
            off += n
        for n in n_to:
            to_at.append(off)
            off += n
        acc_at = 0 if layout == "head" else off
        flag_at = acc_at + 24
        view = lambda at, n: flat.body[at:at + n]
        for h in range(3):
            d.p[h], d.dp[h], d.tobj[h] = p[h].data_ptr(), flat.ptr(dp_at[h]), flat.ptr(to_at[h])
        d.acc, d.flag = flat.ptr(acc_at), flat.ptr(flag_at)
        dps = [view(dp_at[h], n_dp[h]) for h in range(3)]
        tos = [view(to_at[h], n_to[h]) for h in range(3)]
        flag = view(flag_at, 1)
    else:
        for h in range(3):
            bufs["dp%d" % h], bufs["tobj%d" % h] = Guarded(n_dp[h]), Guarded(n_to[h])
            d.p[h], d.dp[h], d.tobj[h] = p[h].data_ptr(), bufs["dp%d" % h].ptr(), bufs["tobj%d" % h].ptr()
        bufs["acc"], bufs["flag"] = Guarded(24), Guarded(1)
        d.acc, d.flag = bufs["acc"].ptr(), bufs["flag"].ptr()
        dps = [bufs["dp%d" % h].body for h in range(3)]
        tos = [bufs["tobj%d" % h].body for h in range(3)]
        flag = bufs["flag"].body
    assert d.acc % 8 == 0
    rc = L.load().dyk_yolo_loss(ctypes.byref(d), ctypes.byref(t), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    counts = bufs["counts"].body.cpu().tolist()
    out = bufs["out"].body.view(torch.float32).cpu()
    res = {k: out[i] for i, k in enumerate(SCALARS)}
    res["grads"] = [dps[h].view(torch.float32).cpu().view(p[h].shape) for h in range(3)]
    res["tobj"] = [tos[h].view(torch.float32).cpu().view(p[h].shape[:4]) for h in range(3)]
    res.update(flag=int(flag.cpu()[0]), counts=counts, bufs=bufs, cap=cap)
    return res


@pytest.mark.parametrize("kind,seed", [("crowded", 1), ("chunk_edges", 14)], ids=["crowded-1", "chunk_edges-14"])
def test_c_abi_three_buffer_layouts_agree_and_stay_inside_their_buffers(kind, seed):
    """head: acc | flag | pad | dp.. | tobj..   tail: dp.. | tobj.. | acc | flag   separate: one allocation per buffer.  Every
    buffer starts as NaN bits between guard bands: whatever the call does not clear or write shows."""
    assert (kind, seed) in FAMILIES
    f = loss_family(kind, seed)
    res = {layout: _abi_call(f, layout) for layout in ("head", "tail", "separate")}
    r = f["r64"]
    bound = oloss.loss_bound(oloss.loss_errors(f["r32"], r))
    for layout, got in res.items():
        assert all(b.intact() for b in got["bufs"].values()), layout
        assert got["flag"] == 0 and got["counts"] == [len(v) for v in r["valid"]], layout
        cap = got["cap"]
        # the match lists are written up to counts[h] and not behind
        idx = got["bufs"]["indices"].body.view(torch.int64).view(3, 4, cap).cpu()
        tcl = got["bufs"]["tcls"].body.view(torch.int64).view(3, cap).cpu()
        tbx = got["bufs"]["tbox"].body.view(3, cap, 4).cpu()
        fill64 = (FILL_BITS << 32) | FILL_BITS
        for h, n in enumerate(got["counts"]):
            assert torch.equal(idx[h, :, :n], torch.stack(list(r["matches"][2][h]))), (layout, h)
            assert torch.equal(tcl[h, :n], r["matches"][0][h]), (layout, h)
            assert bool((idx[h, :, n:] == fill64).all()) and bool((tcl[h, n:] == fill64).all()) and bool((tbx[h, n:] == FILL_BITS).all())
        err = oloss.loss_errors(got, r)
        for k in err:
            assert err[k][0] <= bound[k][0] and err[k][1] <= bound[k][1], (layout, k, err[k], bound[k])
    ref = res["head"]
    for layout in ("tail", "separate"):
        got = res[layout]
        for k in SCALARS:
            assert torch.equal(_bits(got[k].reshape(1)), _bits(ref[k].reshape(1))), (layout, k)
        for h in range(3):
            single = _cell_counts(f, h) <= 1
            assert torch.equal(_bits(got["tobj"][h]), _bits(ref["tobj"][h])), (layout, h)
            assert torch.equal(_bits(got["grads"][h][..., 4]), _bits(ref["grads"][h][..., 4])), (layout, h)
            assert torch.equal(_bits(got["grads"][h])[single], _bits(ref["grads"][h])[single]), (layout, h)
    # and the product's own path (dyk/detect.py, head layout) gives the same bits
    own = _run(kind, seed)[0]
    for k in SCALARS:
        assert torch.equal(_bits(own[k].reshape(1)), _bits(ref[k].reshape(1))), k
    for h in range(3):
        assert torch.equal(_bits(own["tobj"][h]), _bits(ref["tobj"][h])), h
