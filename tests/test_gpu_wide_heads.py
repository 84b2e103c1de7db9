"""Detection heads wider than 32 channels on the GPU: the one-launch eval head against the two launches it replaces (bit for bit),
every tile configuration the conv front end offers for the head conv, its data gradient and its weight gradient at the new
shapes, and models.YOLO at classes = 5 / 6 / 20 / 27 / 80 in every mode against the oracle (tests/wide_head_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wide_head_cases as WC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
ANCHORS = [1.25, 1.625, 2.0, 3.75, 4.125, 2.875, 0.5, 0.75, 7.0, 9.5, 3.0, 3.0, 1.0, 2.0, 5.0, 6.0]


@pytest.fixture(scope="module")
def cfg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide_heads_gpu")


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-12))


# ------------------------------------------------------------------------------------------ kernel equivalence
def _head_y(B, ny, nx, na, no, ld, seed):
    """head conv output rows: logits ~ N(0, 3), +-88 and +-0 planted in box, objectness and class channels of every anchor (expf
    saturates in both directions), NaN in the pad channels (nobody may read them)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, ny, nx, ld, generator=g) * 3.0
    special = [88.0, -88.0, 0.0, -0.0, 88.7, -104.0]
    k = 0
    for a in range(na):
        for o in list(range(6)) + [no - 1]:
            for v in special:
                y[k % B, (k // B) % ny, (k // (B * ny)) % nx, a * no + o] = v
                k += 1
    y[..., na * no:] = float("nan")
    return y.cuda()


def _framed(n):
    buf = torch.full((n + 128,), SENTINEL, device="cuda")
    return buf, buf[64:64 + n]


def _decode_both_ways(y, B, ny, nx, na, no, ld, rows_total, r0, v4, stride):
    from dyk import lib as L, ops
    h = L.load()
    st = ops._stream()
    n_p, n_io = B * na * ny * nx * no, B * rows_total * no
    out = []
    for fused in (False, True):
        pbuf, p = _framed(n_p)
        iobuf, io = _framed(n_io)
        d = L.DykHeadDecodeDesc() if fused else L.DykDecodeDesc()
        d.p, d.io = p.data_ptr(), io.data_ptr()
        d.B, d.na, d.ny, d.nx, d.no = B, na, ny, nx, no
        d.rows_total, d.row_offset, d.v4, d.stride = rows_total, r0, v4, stride
        for q in range(2 * na):
            d.anchor_vec[q] = ANCHORS[q]
        if fused:
            d.y, d.ld = y.data_ptr(), ld
            L.check(h.dyk_head_decode(ctypes.byref(d), st), "dyk_head_decode")
        else:
            L.check(h.dyk_head_permute_fwd(y.data_ptr(), p.data_ptr(), B, ny, nx, na, no, ld, st), "dyk_head_permute_fwd")
            L.check(h.dyk_yolo_decode(ctypes.byref(d), st), "dyk_yolo_decode")
        out.append((pbuf, iobuf))
    return out


@pytest.mark.parametrize("v4", [0, 1])
@pytest.mark.parametrize("nc", WC.NCS)
def test_head_decode_equals_permute_plus_decode_bit_for_bit(nc, v4):
    """both head maps of the fixture inside ONE io buffer (row_offset 0 and 96) that carries 7 foreign rows at either end: p, the
    head's rows of io, the rest of io and the frames around both buffers, compared as bit patterns"""
    from dyk.plan import head_ld
    na, no = WC.NA, 5 + nc
    ld = head_ld(na * no)
    maps = [(4, 8, 8.0), (2, 4, 16.0)]
    rows_total = 7 + sum(na * ny * nx for ny, nx, _ in maps) + 7
    r0 = 7
    for h, (ny, nx, stride) in enumerate(maps):
        y = _head_y(WC.B, ny, nx, na, no, ld, 100 * nc + h)
        (p0, io0), (p1, io1) = _decode_both_ways(y, WC.B, ny, nx, na, no, ld, rows_total, r0, v4, stride)
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))
        assert torch.equal(io0.view(torch.int32), io1.view(torch.int32))
        # the yardstick itself: frames and foreign rows untouched, the head's rows all written, the planted logits saturate
        io = io1[64:-64].view(WC.B, rows_total, no)
        rows = na * ny * nx
        assert bool((io[:, :r0] == SENTINEL).all()) and bool((io[:, r0 + rows:] == SENTINEL).all())
        assert bool((io1[:64] == SENTINEL).all()) and bool((io1[-64:] == SENTINEL).all())
        assert bool((p1[:64] == SENTINEL).all()) and bool((p1[-64:] == SENTINEL).all())
        mine = io[:, r0:r0 + rows]
        assert not bool((mine == SENTINEL).any()) and not bool(torch.isnan(mine).any())
        assert float(mine[..., 4:].max()) == 1.0 and float(mine[..., 4:].min()) == 0.0
        assert torch.equal(p1[64:-64].view(WC.B, na, ny, nx, no),
                           y[..., :na * no].view(WC.B, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous())
        r0 += rows


def test_head_decode_grid_stride_and_argument_checks():
    """more elements than one pass of the largest grid covers (8192 x 256), odd map sizes; and what the entry point refuses"""
    from dyk import lib as L
    B, ny, nx, na, no, ld = 4, 41, 51, 3, 85, 256
    assert B * na * ny * nx * no > 8192 * 256
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(B, ny, nx, ld, generator=g) * 3.0).cuda()
    rows = na * ny * nx
    (p0, io0), (p1, io1) = _decode_both_ways(y, B, ny, nx, na, no, ld, rows + 3, 3, 1, 32.0)
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(io0.view(torch.int32), io1.view(torch.int32))
    h = L.load()
    d = L.DykHeadDecodeDesc()
    d.y, d.p, d.io = y.data_ptr(), p1.data_ptr(), io1.data_ptr()
    d.B, d.na, d.ny, d.nx, d.no, d.ld, d.rows_total, d.row_offset, d.stride = B, na, ny, nx, no, ld, rows + 3, 3, 32.0
    for field, bad in (("ld", 254), ("na", 9), ("no", 4), ("row_offset", 4), ("row_offset", -1), ("y", None), ("io", None)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert h.dyk_head_decode(ctypes.byref(d), None) == -1, field
        setattr(d, field, keep)


# ------------------------------------------------------------------------------------------ conv front end at the head shapes
_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _tight(t, spare=64):
    """a channels-last tensor with `spare` zero elements behind its last pixel (tight rows: the K step over-reads them)"""
    flat = torch.zeros(t.numel() + spare, dtype=t.dtype, device=t.device)
    flat[:t.numel()] = t.reshape(-1)
    return flat[:t.numel()].view(t.shape)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("cin", [48, 64])
@pytest.mark.parametrize("nc", WC.WIDE)
def test_every_conv_route_takes_the_head_shapes(nc, cin, dtype):
    """Cout = 33 / 75 / 96 / 255 over 48 (K padded to 64) and 64 input channels, the fixture's larger head map: the head conv
    (bias, fp32 rows of head_ld channels), its data gradient (K = head_ld, zero weight rows under the pad) and its weight gradient,
    under EVERY tune word the plan's tuner would try for them.  Reference: the same product of the rounded operands in float64.
    Bounds: fp32 accumulation of K <= 256 products, K * 2^-24 of sum |products| <= 2e-5 of the output's scale; a 16-bit output adds
    one rounding, 2^-8 (bf16) / 2^-11 (fp16) of the scale."""
    from dyk import lib as L, ops
    from dyk.plan import _WGRAD_CANDIDATES, _conv_candidates, head_ld
    dt = _DT[dtype]
    cout, (ny, nx) = WC.NA * (5 + nc), (4, 8)
    ld = head_ld(cout)
    g = torch.Generator().manual_seed(1000 * nc + cin)
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    bias = torch.randn(cout, generator=g)
    x = torch.randn(WC.B, cin, ny, nx, generator=g).to(dt).float()
    dy = torch.zeros(WC.B, ld, ny, nx)
    dy[:, :cout] = torch.randn(WC.B, cout, ny, nx, generator=g)
    dy = dy.to(dt).float()
    wr = w.to(dt).double()
    ref_y = F.conv2d(x.double(), wr, bias.double())
    ref_dx = F.conv_transpose2d(dy[:, :cout].double(), wr)
    ref_dw = torch.einsum("bohw,bihw->oi", dy[:, :cout].double(), x.double())
    xd = _tight(ops.to_nhwc(x.cuda(), dt))
    cin_k = -(-cin // 32) * 32
    wp = ops.pack_weight(w.cuda(), dt, cin_pad=cin_k)
    bias_d = bias.cuda()
    h = L.load()
    st = ops._stream()
    worst = {}
    # ---- head conv: every candidate writes its own output
    out = torch.full((WC.B, ny, nx, ld), SENTINEL, device="cuda")
    d = ops.make_conv_desc(xd, wp, out, Hi=ny, Wi=nx, Cin=cin_k, Cout=cout, Hg=ny, Wg=nx, Ho=ny, Wo=nx, taps=[(0, 0, 0)],
                           shift=bias_d, out_f32=True, ldx=cin, ldy=ld)
    cands = _conv_candidates(d)
    assert len(cands) >= (8 if dtype == "fp32" else 24)
    for c in cands:
        out.fill_(SENTINEL)
        d.tune = c
        L.check(h.dyk_conv_igemm(ctypes.byref(d), st), "head conv, tune %#x" % c)
        assert bool((out[..., cout:] == SENTINEL).all()), "tune %#x wrote the pad channels" % c
        worst["fwd"] = max(worst.get("fwd", 0.0), _rel(out[..., :cout].permute(0, 3, 1, 2).cpu(), ref_y))
    assert worst["fwd"] <= 2e-5, worst
    if dtype == "fp16":
        return                                  # inference type: no gradients
    # ---- data gradient: K = ld over rows of ld elements
    dyd = ops.to_nhwc(dy.cuda(), dt)
    wpt = ops.pack_weight(w.cuda(), dt, transposed=True, cout_pad=ld)
    dx = torch.zeros((WC.B, ny, nx, cin), dtype=dt, device="cuda")
    d = ops.make_conv_desc(dyd, wpt, dx, Hi=ny, Wi=nx, Cin=ld, Cout=cin, Hg=ny, Wg=nx, Ho=ny, Wo=nx, taps=[(0, 0, 0)])
    for c in _conv_candidates(d):
        dx.zero_()
        d.tune = c
        L.check(h.dyk_conv_igemm(ctypes.byref(d), st), "head data gradient, tune %#x" % c)
        worst["dgrad"] = max(worst.get("dgrad", 0.0), _rel(dx.float().permute(0, 3, 1, 2).cpu(), ref_dx))
    assert worst["dgrad"] <= 2e-5 + (2.0 ** -8 if dtype == "bf16" else 0.0), worst
    # ---- weight gradient
    for c in _WGRAD_CANDIDATES:
        dw = ops.conv2d_wgrad(xd, dyd, 1, 1, 0, Cin=cin, Cout=cout, tune=c)
        worst["wgrad"] = max(worst.get("wgrad", 0.0), _rel(dw[0].cpu(), ref_dw))
    assert worst["wgrad"] <= 2e-5, worst
    print("nc %d cin %d %s: worst deviation %s" % (nc, cin, dtype, worst))


# ------------------------------------------------------------------------------------------ models.YOLO
def _model(cfg, sd, dtype):
    from models import YOLO
    torch.manual_seed(0)
    m = YOLO(cfg)
    m.load_state_dict(sd)
    m.dyk_dtype = dtype
    return m.cuda()


def _ops(m):
    plan = next(iter(m.engine.plans.values()))
    return plan, [op for op, _ in plan.fwd]


# fp32 / bf16: the tolerances of test_mismatched_channel_shortcuts_match_reference for this network family.  fp16: the
# whole-model statement of tests/test_gpu_fp16.py -- a quarter of the bf16 deviation (2^-3 = the ratio of the rounding steps,
# x 2 for the max-norm) -- applied to the bf16 bound.
EVAL_TOL = {"fp32": 2e-4, "bf16": 4e-2, "fp16": 0.25 * 4e-2}


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("v4", [False, True], ids=["v3", "v4"])
@pytest.mark.parametrize("nc", WC.NCS)
def test_eval_matches_the_oracle_and_nms_keeps_the_same_rows(cfg_dir, nc, v4, dtype):
    from build_utils.utils import non_max_suppression
    from dyk import detect, lib as L
    from oracle import nms as onms
    o = WC.oracle(cfg_dir, nc, v4)
    m = _model(o["cfg"], o["sd"], dtype).eval()
    with torch.no_grad():
        io, p = m(WC.inputs().cuda())
    plan, ops = _ops(m)
    wide = nc in WC.WIDE
    assert ops.count(L.OP_HEAD_DECODE) == (2 if wide else 0) and ops.count(L.OP_YOLO_DECODE) == (0 if wide else 2)
    tol = EVAL_TOL[dtype]
    errs = [_rel(a.cpu(), b) for a, b in zip(p, o["eval_p"])] + [_rel(io.cpu(), o["eval_io"])]
    print("nc %d %s %s: p / io deviation %s" % (nc, "v4" if v4 else "v3", dtype, ["%.2e" % e for e in errs]))
    assert io.shape == o["eval_io"].shape and bool(torch.isfinite(io).all())
    assert max(errs) < tol, errs
    if dtype != "fp32":
        return
    # NMS on the product's own decode output: same kept candidates, same order, same values as the oracle's NMS of it
    # (threshold from the data: the 40 best objectness x class scores of the batch pass it, more label pairs with multi_label)
    best = (io[..., 4:5] * io[..., 5:]).max(-1).values.flatten()
    thr = float(best.sort().values[-40]) * 0.999
    for multi in (False, True):
        ref, rows_ref = onms.non_max_suppression(io.cpu(), thr, 0.5, multi_label=multi, return_indices=True)
        out, rows = detect.non_max_suppression(io, thr, 0.5, multi_label=multi, return_rows=True)
        api = non_max_suppression(io, thr, 0.5, multi_label=multi)
        assert sum(0 if r is None else len(r) for r in rows_ref) > 0
        for b in range(WC.B):
            if ref[b] is None or ref[b].shape[0] == 0:
                assert out[b] is None and api[b] is None
                continue
            assert np.array_equal(out[b].cpu().numpy(), ref[b].numpy()) and np.array_equal(api[b].cpu().numpy(), ref[b].numpy())
            assert rows[b].cpu().tolist() == rows_ref[b].tolist()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("nc", WC.NCS)
def test_training_matches_the_oracles_autograd(cfg_dir, nc, dtype):
    """head tensors, the three loss terms (targets of the first and the last class), the head convs' weight and bias gradients
    element by element and every other parameter gradient by (sum |g|, sum g), at the tolerances of
    test_mismatched_channel_shortcuts_match_reference; the pad channels of the head gradient rows are zero.  Yardstick: the
    oracle's autograd -- in bf16 seeded with the oracle's loss gradient at the bf16 head tensors (see below, and DESIGN.md
    section 14: against the gradient at the oracle's own logits the bf16 cases measure 2.5e-2, 9.4e-3, 1.5e-2, 1.8e-2 and, at nc = 80, 0.316 -- printed for every case)."""
    from build_utils.utils import compute_loss
    from dyk import lib as L
    v4 = nc in (20, 80)                         # both box flavours of the loss over the cases
    o = WC.oracle(cfg_dir, nc, v4)
    m = _model(o["cfg"], o["sd"], dtype).train()
    m.nc, m.hyp, m.gr = nc, WC.hyp(), 1.0
    out = m(WC.inputs().cuda())
    f32 = dtype == "fp32"
    errs = [_rel(a.detach().cpu(), b) for a, b in zip(out, o["train_p"])]
    assert max(errs) < (1e-3 if f32 else 6e-2), errs
    ld = compute_loss(out, WC.targets(nc).cuda(), m)
    got = [ld[k].item() for k in ("box_loss", "obj_loss", "class_loss")]
    (ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]).backward()
    assert int(m._dyk_loss_flag.item()) == 0
    lt = 2e-4 if f32 else 3e-2
    print("nc %d %s: head deviation %s, loss %s (oracle %s)" % (nc, dtype, ["%.2e" % e for e in errs], got, o["loss"]))
    assert all(abs(a - b) <= lt * abs(b) for a, b in zip(got, o["loss"])), (got, o["loss"])
    gt = 5e-3 if f32 else 8e-2
    params = dict(m.named_parameters())
    head_names = ["module_list.%d.Conv2d.%s" % (j - 1, leaf) for j in m.yolo_layers for leaf in ("weight", "bias")]
    # fp32: the oracle's autograd from its own loss.  bf16: the oracle's autograd seeded with the oracle's loss gradient AT the
    # bf16 head tensors (wide_head_cases.oracle_backward_from).  Against the gradient at the oracle's own logits the head conv
    # of the nc = 80 case measured 0.316 of its scale in weight rows 1 and 3 (box y, h of anchor 0) and 0.118 in the same rows of
    # its BIAS gradient, which is a plain fp32 sum of the loss gradient: the loss gradient itself moved.  On the CPU, the oracle's
    # loss gradient moves single bias-gradient elements by up to 0.28 of the scale when its logits move by the 4e-3 of a bf16 head.
    ref_g = o["grads"] if f32 else WC.oracle_backward_from(o, nc, v4, out)
    literal = max(_rel(params[name].grad.cpu(), o["grads"][name]) for name in head_names)
    print("nc %d %s: head conv gradients against the gradient at the oracle's own logits: %.3e" % (nc, dtype, literal))
    for name in head_names:
        g, ref = params[name].grad.cpu(), ref_g[name]
        print("   %s: %.3e of scale" % (name, _rel(g, ref)))
        assert float((g - ref).abs().max()) <= gt * float(ref.abs().max()), (name, _rel(g, ref))
    got_s = np.array([[q.grad.abs().sum().item(), q.grad.sum().item()] for _, q in params.items()])
    ref_s = np.array([[ref_g[k].abs().sum().item(), ref_g[k].sum().item()] for k in params])
    assert np.allclose(got_s[:, 0], ref_s[:, 0], rtol=gt, atol=1e-6), np.abs(got_s[:, 0] / np.maximum(ref_s[:, 0], 1e-12) - 1).max()
    # the head gradient rows as the backward pass left them: channels >= na * no are zero
    plan = next(iter(m.engine.plans.values()))
    torch.cuda.synchronize()
    es, gdt = (4, torch.float32) if f32 else (2, torch.bfloat16)
    n_heads = 0
    for op, d in plan.bwd:
        if op == L.OP_HEAD_PERMUTE_BWD:
            B, ny, nx, na, no, ldh = (d.i[q] for q in range(6))
            assert ldh == WC.expected_ld(nc)
            off = d.p[1] - plan.arenas["grad"].ptr()
            rows = plan.arenas["grad"].tensor[off:off + B * ny * nx * ldh * es].view(gdt).view(B * ny * nx, ldh)
            assert float(rows[:, :na * no].abs().max()) > 0
            assert ldh == na * no or float(rows[:, na * no:].abs().max()) == 0.0
            n_heads += 1
    assert n_heads == 2


@pytest.mark.parametrize("nc", [1, 5])
def test_narrow_heads_are_bit_reproducible_on_the_old_op_list(cfg_dir, nc, monkeypatch):
    from dyk import lib as L
    monkeypatch.setenv("DYK_AUTOTUNE", "0")
    monkeypatch.setenv("DYK_TUNE_CACHE", "0")
    from build_utils.parse_config import parse_model_cfg
    from oracle.model import OracleNet
    cfg = WC.TEMPLATE if nc == 1 else WC.write_cfg(cfg_dir, nc)
    sd = OracleNet(parse_model_cfg(cfg), cfg).synth_state(3)
    res = []
    for _ in range(2):
        m = _model(cfg, sd, "bf16").eval()
        with torch.no_grad():
            io, p = m(WC.inputs().cuda())
        plan, ops = _ops(m)
        assert ops == [18, 32, 18, 1, 18, 1, 1, 21, 18, 1, 1, 21, 25, 25] and L.OP_HEAD_DECODE == 34
        ev = [io.clone()] + [t.clone() for t in p]
        m.train()
        out = m(WC.inputs().cuda())
        sum((t.float() ** 2).mean() for t in out).backward()
        torch.cuda.synchronize()
        res.append(ev + [t.detach().clone() for t in out] + [q.grad.clone() for q in m.parameters()])
    assert len(res[0]) == len(res[1]) and all(torch.equal(a, b) for a, b in zip(*res))
