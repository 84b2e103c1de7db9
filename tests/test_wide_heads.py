"""Detection heads wider than 32 channels, host side (no GPU): the row-width rule, the plans of every class count in both modes
and all compute types (dry compilation), which op decodes which head, the scheduler's access sets of the one-launch head, and
the host-side limits (anchors per head, the class filter of non_max_suppression)."""
import ctypes

import pytest
import torch

import wide_head_cases as WC


@pytest.fixture(scope="module")
def cfg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide_heads")


def _plan(cfg, dtype, training):
    from dyk.params import ParamStore
    from dyk.plan import compile_plan
    from models import YOLO
    torch.manual_seed(0)
    m = YOLO(cfg)
    st = ParamStore(m)
    st.adopt(torch.device("cpu"))
    return m, st, compile_plan(m, st, WC.B, WC.H, WC.W, dtype, training, torch.device("cpu"), dry=True)


def test_width_rule():
    from dyk.plan import HEAD_LD, head_ld
    assert HEAD_LD == 32
    for c in range(1, 33):
        assert head_ld(c) == 32
    for c in range(33, 600):
        ld = head_ld(c)
        assert ld % 32 == 0 and c <= ld < c + 32
    assert [head_ld(WC.NA * (5 + nc)) for nc in WC.NCS] == [32, 64, 96, 96, 256] == [WC.expected_ld(nc) for nc in WC.NCS]
    assert head_ld(18) == 32 and head_ld(255) == 256 and head_ld(256) == 256 and head_ld(257) == 288


@pytest.mark.parametrize("nc", WC.NCS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_eval_plan_compiles_and_picks_the_decode_by_width(cfg_dir, nc, dtype):
    from dyk import lib as L
    m, st, plan = _plan(WC.write_cfg(cfg_dir, nc), dtype, False)
    ops = [op for op, _ in plan.fwd]
    no, ld = 5 + nc, WC.expected_ld(nc)
    maps = [(WC.H // 8, WC.W // 8), (WC.H // 16, WC.W // 16)]
    assert [tuple(p.shape) for p in plan.p_out] == [(WC.B, WC.NA, ny, nx, no) for ny, nx in maps]
    rows = [WC.NA * ny * nx for ny, nx in maps]
    assert tuple(plan.io.shape) == (WC.B, sum(rows), no)
    heads = [d for op, d in plan.fwd if op == L.OP_CONV and d.flags & L.EPI_OUT_F32]
    assert [(d.Cout, d.ldy) for d in heads] == [(WC.NA * no, ld)] * 2
    assert [d.ldx for d in heads] == [48, 64] and [d.Cin for d in heads] == [64, 64]      # K = the input channels rounded up to 32
    if nc in WC.WIDE:
        assert ops.count(L.OP_HEAD_DECODE) == 2 and ops.count(L.OP_YOLO_DECODE) == 0 and ops.count(L.OP_HEAD_PERMUTE_FWD) == 0
        assert ops[-2:] == [L.OP_HEAD_DECODE] * 2
        dec = [d for op, d in plan.fwd if op == L.OP_HEAD_DECODE]
        assert [(d.B, d.na, d.ny, d.nx, d.no, d.ld, d.rows_total, d.row_offset, d.v4) for d in dec] == [
            (WC.B, WC.NA, ny, nx, no, ld, sum(rows), r0, 0) for (ny, nx), r0 in zip(maps, (0, rows[0]))]
        assert [d.stride for d in dec] == [8.0, 16.0]
        for d, h, p in zip(dec, heads, plan.p_out):
            assert d.y == h.y and d.p == p.data_ptr() and d.io == plan.io.data_ptr()
            assert list(d.anchor_vec)[:6] == [float(v) for v in m.module_list[m.yolo_layers[dec.index(d)]].anchor_vec.reshape(-1)]
    else:
        assert ops.count(L.OP_HEAD_DECODE) == 0 and ops.count(L.OP_YOLO_DECODE) == 2 and ops.count(L.OP_HEAD_PERMUTE_FWD) == 2
        assert ops[-2:] == [L.OP_YOLO_DECODE] * 2


@pytest.mark.parametrize("nc", WC.NCS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_training_plan_compiles_with_the_head_gradient_in_padded_rows(cfg_dir, nc, dtype):
    from dyk import lib as L
    m, st, plan = _plan(WC.write_cfg(cfg_dir, nc), dtype, True)
    no, ld = 5 + nc, WC.expected_ld(nc)
    fops, bops = [op for op, _ in plan.fwd], [op for op, _ in plan.bwd]
    assert fops.count(L.OP_HEAD_PERMUTE_FWD) == 2 and fops.count(L.OP_HEAD_DECODE) == 0 and fops.count(L.OP_YOLO_DECODE) == 0
    assert bops.count(L.OP_HEAD_PERMUTE_BWD) == 2
    es = 4 if dtype == torch.float32 else 2
    grad = plan.arenas["grad"]
    for op, d in plan.bwd:
        if op == L.OP_HEAD_PERMUTE_BWD:
            assert (d.i[3], d.i[4], d.i[5]) == (WC.NA, no, ld)
            # the head gradient: rows of `ld` elements that the head conv's weight gradient (lddy) and its data gradient
            # (K = Cin = ldx = ld) read
            wg = [w for o, w in plan.bwd if o == L.OP_WGRAD and w.dy == d.p[1]]
            dg = [c for o, c in plan.bwd if o == L.OP_CONV and c.x == d.p[1]]
            assert len(wg) == 1 and (wg[0].Cout, wg[0].lddy) == (WC.NA * no, ld)
            assert len(dg) == 1 and (dg[0].Cin, dg[0].ldx) == (ld, ld)
            # ... inside a block of the gradient arena that holds B * ny * nx such rows
            off = d.p[1] - grad.ptr()
            blocks = dict(grad.blocks)
            assert off in blocks and blocks[off] >= d.i[0] * d.i[1] * d.i[2] * ld * es
    # the data gradient's weight pack has `ld` columns per input channel, zero under the pad
    cw = st.alloc_compute(dtype)
    for j in m.yolo_layers:
        name = "module_list.%d.Conv2d.weight" % (j - 1)
        assert (name in cw["bwd_pad_off"]) == (WC.NA * no != ld)


def test_narrow_plans_keep_their_op_list(cfg_dir):
    """nc = 1 (the template itself) and nc = 5 (30 channels): the ops of every head are the two launches they always were"""
    from dyk import lib as L
    for cfg in (WC.TEMPLATE, WC.write_cfg(cfg_dir, 5)):
        _, _, plan = _plan(cfg, torch.bfloat16, False)
        ops = [op for op, _ in plan.fwd]
        assert L.OP_HEAD_DECODE not in ops and ops.count(L.OP_YOLO_DECODE) == 2
        # the op list of the template's eval plan as it was before heads could be wider (op codes are ABI: they never move)
        assert ops == [L.OP_BN_FOLD, L.OP_STEM_FWD, L.OP_BN_FOLD, L.OP_CONV, L.OP_BN_FOLD, L.OP_CONV,
                       L.OP_CONV, L.OP_HEAD_PERMUTE_FWD, L.OP_BN_FOLD, L.OP_CONV, L.OP_CONV, L.OP_HEAD_PERMUTE_FWD,
                       L.OP_YOLO_DECODE, L.OP_YOLO_DECODE] == [18, 32, 18, 1, 18, 1, 1, 21, 18, 1, 1, 21, 25, 25]
        for op, d in plan.fwd:
            if op == L.OP_HEAD_PERMUTE_FWD:
                assert d.i[5] == 32
            if op == L.OP_CONV and d.flags & L.EPI_OUT_F32:
                assert d.ldy == 32


def test_scheduler_knows_the_one_launch_head(cfg_dir):
    """read set = the head conv's output block, write sets = p and io: each decode follows its head conv, and the schedule of the
    whole list builds without a barrier at the heads"""
    from dyk import lib as L, sched
    _, st, plan = _plan(WC.write_cfg(cfg_dir, 80), torch.bfloat16, False)
    mem = sched.Memory(plan, st)
    deps = sched.dependencies(plan.fwd, mem, plan)
    idx = {ctypes.addressof(d): k for k, (op, d) in enumerate(plan.fwd)}
    heads = [d for op, d in plan.fwd if op == L.OP_CONV and d.flags & L.EPI_OUT_F32]
    decs = [(k, d) for k, (op, d) in enumerate(plan.fwd) if op == L.OP_HEAD_DECODE]
    assert len(decs) == 2
    for (k, d), h in zip(decs, heads):
        R, W, barrier = sched.accesses(L.OP_HEAD_DECODE, d, mem, plan)
        assert not barrier and len(R) == 1 and len(W) == 2
        assert idx[ctypes.addressof(h)] in deps[k]
    assert decs[0][0] in deps[decs[1][0]]            # both write io (tracked as one interval)
    assert sched.estimate_cost_us(L.OP_HEAD_DECODE, decs[0][1], plan) > 4.0


def test_more_anchors_than_the_decode_takes_is_refused_by_name(cfg_dir):
    text = open(WC.TEMPLATE).read().replace("mask = 3,4,5", "mask = 0,1,2,3,4,5,0,1,2").replace("filters=18", "filters=54")
    text = text.replace("mask = 0,1,2\n", "mask = 0,1,2,3,4,5,0,1,2\n")
    path = str(cfg_dir / "tiny_nine_anchors.cfg")
    with open(path, "w") as f:
        f.write(text)
    with pytest.raises(NotImplementedError, match=r"9 anchors \(layer 4\)"):
        _plan(path, torch.float32, False)


def test_class_filter_longer_than_the_descriptor_is_a_value_error():
    from build_utils.utils import non_max_suppression
    from dyk import detect
    pred = torch.zeros(1, 4, 25)
    for fn in (non_max_suppression, detect.non_max_suppression):
        with pytest.raises(ValueError, match="at most 16"):
            fn(pred, 0.1, 0.6, classes=list(range(17)))
    assert detect.NMS_MAX_CLASSES == len(detect.L.DykNmsDesc().classes)
