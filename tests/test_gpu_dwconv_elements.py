"""csrc/dwconv.hip held to the fp64 reference of oracle/dwconv.py, element by element, on every dispatch path.

Every launch writes into a buffer pre-filled with a sentinel: rows of ld = C + 16 elements (padding channels beyond C) between
guard rows.  Afterwards the guards and the padding are bit-identical and every element in range is inside its derived bound
(oracle/dwconv.py; tests/test_dwconv_reference.py shows on the CPU that the bounds admit a correct fp32 implementation and flag
seven kinds of subtly wrong kernel).  The cases are those of tests/dwconv_cases.py; `view` cases read x / dy as channel slices
[8 : 8 + C] of a buffer with ld = C + 24 (the weight gradient: dy as [16 : 16 + C] of ld = C + 40, so that ldx != ldy there too).

Kernel instantiations dwconv.hip launches, and a case that reaches each (bf16 unless said otherwise):
    dwconv_kernel<bf16, fwd>            c264_k3p1s2_9x12 (second channel block, one active vector), c24_k3p1s3_12x11, c72_k1_5x9,
                                        c8_k2p1_6x7, c16_k4p1_9x8, c24_k7p3_9x17, c264_k1_683x1 (two image rows per workgroup)
    dwconv_kernel<float, fwd>           every case in f32: c4_k3p1_7x9, c12_k5p2s2_9x8, ...
    dwconv_kernel<f16, fwd>             the stride-2 / stride-3 / k 1, 2, 4, 7 cases in f16
    dwconv_kernel<bf16, grad>           c24_k3p1s3_12x11, c72_k1_5x9, c8_k2p1_6x7, c16_k4p1_9x8, c24_k7p3_9x17
    dwconv_kernel<float, grad>          every data-gradient case in f32
    dwconv_tile_kernel<3, fwd, bf16>    c8_k3p1_66x17, c56_k3p1_10x16, c72_k3p1_1x17, c184_k3p1_1x1, c8_k3p0_5x20; `pre` k 3
    dwconv_tile_kernel<5, fwd, bf16>    c24_k5p2_23x17, c64_k5p1_9x3, c264_k5p0_6x21, c16_k5p2_35x33; `pre` k 5
    dwconv_tile_kernel<3 | 5, fwd, f16> the same cases in f16
    dwconv_tile_kernel<3 | 5, grad>     the same cases, data gradient (pad' = k - 1 - pad: 1, 2 at k 3; 2, 3, 4 at k 5)
    dwconv_s2_dgrad_kernel<3, bf16>     c264_k3p1s2_9x12, c24_k3p0s2_8x10 (last row and column exact zeros), c8_k3p2s2_6x5
    dwconv_s2_dgrad_kernel<5, bf16>     c72_k5p2s2_11x10, c16_k5p0s2_10x10 (last row and column exact zeros), c8_k5p1s2_9x12
    dwconv_wgrad_kernel<bf16, 1>        c72_k1_5x9                       (strip path)
    dwconv_wgrad_kernel<bf16, 3>        c264_k3p1s2_9x12, c24_k3p0s2_8x10, c8_k3p2s2_6x5, c24_k3p1s3_12x11; `pre` stride 2   (per-pixel path)
    dwconv_wgrad_kernel<bf16, 5>        c72_k5p2s2_11x10, c16_k5p0s2_10x10, c8_k5p1s2_9x12; `pre` stride 2                    (per-pixel path)
    dwconv_wgrad_kernel<bf16, 7>        c24_k7p3_9x17, c8_k7p3_60x5 (two image rows per workgroup)                            (strip path)
    dwconv_wgrad_kernel<float, 1|3|5|7> c72_k1_5x9 | c8_k3p1_66x17, c4_k3p1_7x9 | c24_k5p2_23x17, c12_k5p2s2_9x8 | c24_k7p3_9x17 in f32
    dwconv_wgrad_tile_kernel<3, plain>  c8_k3p1_66x17, ..., c520_k3p1_2x17 (two tiles per workgroup)
    dwconv_wgrad_tile_kernel<5, plain>  c24_k5p2_23x17, ..., c960_k5p2_9x17 (two tiles per workgroup)
    dwconv_wgrad_tile_kernel<3 | 5, pre> test_pre_is_bit_identical_to_the_two_launch_form
The fused BatchNorm-backward data gradient (DykDwDesc.res) keeps its own test in tests/test_gpu_conv.py.

Every test prints `DWRATIO <what> <dtype> <largest error / bound> <case>`; DESIGN.md ("Depthwise kernels against fp64") records the
largest per op and type."""
import ctypes

import pytest
import torch

from dwconv_cases import ACTS, BY_ID, const_problem, matrix, out_hw, pre_inputs, problem
from oracle import dwconv as O

pytestmark = pytest.mark.gpu

SENTINEL = 1984.0                  # representable in bf16 and fp16
UNSUPPORTED = -3                   # DYK_ERR_UNSUPPORTED
PAD_C = 16                         # padding channels of every output row
GUARD_ROWS = 4


def _lib():
    from dyk import lib as L
    return L.load()


class Buf:
    """a channels-last tensor [B, H, W, C] as the channel slice [off : off + C] of rows of `ld` elements, between guard rows, all of
    it filled with the sentinel; .t is what the kernels get"""

    def __init__(self, B, H, W, C, dtype, ld=None, off=0):
        ld = ld or C + PAD_C
        n, g = B * H * W * ld, GUARD_ROWS * ld
        self.flat = torch.full((g + n + g,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.flat[g:g + n].view(B, H, W, ld)[..., off:off + C]
        m = torch.zeros(g + n + g, dtype=torch.bool)
        m[g:g + n].view(B, H, W, ld)[..., off:off + C] = True
        self.inside = m
        self.before = None

    def put(self, nchw):
        self.t.copy_(nchw.permute(0, 2, 3, 1).to(self.t.dtype))
        return self

    def arm(self):
        self.before = self.flat.clone()
        return self

    def get(self):
        return self.t.cpu().permute(0, 3, 1, 2).double()

    def assert_outside_untouched(self, everything=False):
        """guards and padding channels (everything: the tensor's own elements too) are bit-identical to what arm() saw"""
        iv = {2: torch.int16, 4: torch.int32, 8: torch.int64}[self.flat.element_size()]
        a, b = self.flat.cpu().view(iv), self.before.cpu().view(iv)
        out = torch.ones_like(self.inside) if everything else ~self.inside
        assert torch.equal(a[out], b[out]), "%d elements that must stay as they were have been written" % int((a[out] != b[out]).sum())

    def assert_untouched(self):
        self.assert_outside_untouched(everything=True)


def _in_buf(c, dtype, nchw, second=False):
    """an input: tight rows, or (view cases) a channel slice at a 16-byte-aligned non-zero offset of wider rows -- [8 : 8 + C] of
    C + 24, and for the second input of a launch (dy of the weight gradient) [16 : 16 + C] of C + 40, so that ldx != ldy"""
    B, C, H, W = nchw.shape
    if not c.view:
        return Buf(B, H, W, C, dtype, ld=C).put(nchw)
    return (Buf(B, H, W, C, dtype, ld=C + 40, off=16) if second else Buf(B, H, W, C, dtype, ld=C + 24, off=8)).put(nchw)


def _desc(x, y, w, c):
    from dyk import ops
    return ops._dw_desc(x, y, w, c.k, c.s, c.pad, c.C)


def _sync_ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)
    torch.cuda.synchronize()


def _report(what, dt, ratio, bad, case_id):
    print("DWRATIO %s %s %.5f %s" % (what, dt, ratio, case_id))
    assert bad == 0 and ratio <= 1.0, "%s %s %s: %d elements outside their bound, largest error / bound %.3f" % (what, dt, case_id, bad, ratio)


def _tiled(c, dt):
    return c.s == 1 and c.k in (3, 5) and dt in ("bf16", "f16")


def _stats_buf(slots, C):
    st = torch.full((slots + 2, 2, C), SENTINEL, dtype=torch.float64, device="cuda")
    st[1:1 + slots] = 0
    return st


def _run_forward(p, dt, slots):
    c, r = p.case, p.ref
    Ho, Wo = out_hw(c)
    xb = _in_buf(c, p.dtype, p.x).arm()
    yb = Buf(c.B, Ho, Wo, c.C, p.dtype).arm()
    wd = p.w.cuda()
    d = _desc(xb.t, yb.t, wd, c)
    assert _lib().dyk_dwconv_tile_ok(ctypes.byref(d)) == (1 if _tiled(c, dt) else 0)
    st = None
    if slots:
        st = _stats_buf(slots, c.C)
        d.stats, d.stats_slots = st[1:].data_ptr(), slots
    _sync_ok(_lib().dyk_dwconv_fwd(ctypes.byref(d), None), "dyk_dwconv_fwd")
    xb.assert_untouched()
    yb.assert_outside_untouched()
    tgt, b = O.out_bound(r.y, r.A_y, r.T, p.dtype)
    _report("fwd", dt, *O.check(yb.get(), tgt, b), c.id)
    if slots:
        h = st.cpu()
        assert bool((h[0] == SENTINEL).all()) and bool((h[-1] == SENTINEL).all()), "statistics written outside their slots"
        s = h[1:1 + slots].sum(0)
        b1, b2 = O.stats_bound(r)
        _report("s1", dt, *O.check(s[0], r.S1, b1), c.id)
        _report("s2", dt, *O.check(s[1], r.S2, b2), c.id)


@pytest.mark.parametrize("case_id,dt", matrix("f"))
def test_forward(case_id, dt):
    p = problem(case_id, dt)
    _run_forward(p, dt, 0 if dt == "f16" else p.case.slots)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2)])
def test_forward_statistics_come_from_the_accumulators(k, stride):
    """the constant field (tests/dwconv_cases.py): sums of the STORED bf16 values miss the bounds 15- and 33-fold.  Tiled kernel
    (stride 1) and generic kernel (stride 2)"""
    _run_forward(const_problem(k, stride), "bf16", 1)


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("case_id,dt", matrix("d"))
def test_data_gradient(case_id, dt, accumulate):
    p = problem(case_id, dt)
    c, r = p.case, p.ref
    gb = _in_buf(c, p.dtype, p.dy).arm()
    ob = Buf(c.B, c.H, c.W, c.C, p.dtype)
    if accumulate:
        ob.put(p.old)
    ob.arm()
    wd = p.w.cuda()
    d = _desc(ob.t, gb.t, wd, c)
    d.flags = 1 if accumulate else 0
    _sync_ok(_lib().dyk_dwconv_dgrad(ctypes.byref(d), None), "dyk_dwconv_dgrad")
    gb.assert_untouched()
    ob.assert_outside_untouched()
    tgt, b = O.out_bound(r.dx, r.A_dx, r.T, p.dtype, old=p.old if accumulate else None)
    got = ob.get()
    if not accumulate:
        assert bool((got[r.A_dx == 0] == 0).all()), "pixels no gradient reaches are not exact zeros"
    _report("dgrad+" if accumulate else "dgrad", dt, *O.check(got, tgt, b), c.id)


def _wgrad_geometry(c):
    """(tiles, channel groups, workgroups per channel group = planes) of the persistent tiled weight gradient: at most 512
    workgroups per launch, the tiles dealt evenly over the rounds (dw_route_wgrad)"""
    cv = c.C // 8
    groups = (cv + 7) // 8
    ct = -(-cv // groups)
    th = (256 // ct) // 4
    Ho, Wo = out_hw(c)
    tiles = c.B * -(-Ho // th) * -(-Wo // 16)
    p0 = min(max(512 // groups, 1), tiles)
    rounds = -(-tiles // p0)
    return tiles, groups, -(-tiles // rounds)


def _wgrad_row_planes(c, dt):
    """workgroup rows (= planes) of the row kernel: image rows of the output, capped at 768 / k workgroups per launch (dw_route_rows)"""
    cv = c.C // (4 if dt == "f32" else 8)
    cvb = 1
    while cvb < cv and cvb < 32:
        cvb *= 2
    gx = -(-cv // cvb)
    return min(c.B * out_hw(c)[0], max((768 // c.k) // gx, 1))


def _run_wgrad(p, dt, part_shift=0):
    c, r = p.case, p.ref
    kk = c.k * c.k
    xb = _in_buf(c, p.dtype, p.x).arm()
    gb = _in_buf(c, p.dtype, p.dy, second=True).arm()
    dwb = Buf(1, 1, kk, c.C, torch.float32, ld=c.C)
    dwb.t.zero_()
    dwb.arm()
    d = _desc(xb.t, gb.t, None, c)
    assert (d.ldx != d.ldy) == c.view                  # view cases: x and dy of different row widths
    d.dw = dwb.t.data_ptr()
    bound = O.dw_bound(r)
    if part_shift == 0:
        # atomic mode: workgroups add their sums onto dw
        _sync_ok(_lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad")
        dwb.assert_outside_untouched()
        _report("wgrad", dt, *O.check(dwb.t.cpu().view(kk, c.C), r.dw, bound), c.id)
        dwb.t.zero_()
        dwb.arm()
    # plane mode: one partial plane per workgroup row, plain stores
    rows = _lib().dyk_dwconv_wgrad_rows(ctypes.byref(d))
    assert rows >= 1
    if _tiled(c, dt):
        # the plane count pins the dispatch: the persistent tiled kernel, not a quiet fall-back to the row kernel
        tiles, groups, planes = _wgrad_geometry(c)
        assert rows == planes and rows <= tiles, (rows, planes, tiles)
        if c.id in ("c960_k5p2_9x17", "c520_k3p1_2x17"):
            assert rows < tiles and rows * groups <= 512, "this case is meant to walk several tiles per workgroup"
    else:
        assert rows == _wgrad_row_planes(c, dt), (rows, _wgrad_row_planes(c, dt))
    n = rows * kk * c.C
    runs = []
    for _ in range(2):
        flat = torch.full((64 + n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        part = flat[64 + part_shift:64 + part_shift + n]
        part.fill_(float("nan"))
        before = flat.clone()
        d.part = part.data_ptr()
        _sync_ok(_lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad(planes)")
        h = flat.cpu()
        assert torch.equal(h[:64 + part_shift], before.cpu()[:64 + part_shift]) and torch.equal(h[64 + part_shift + n:], before.cpu()[64 + part_shift + n:])
        planes = h[64 + part_shift:64 + part_shift + n].view(rows, kk, c.C)
        assert not bool(torch.isnan(planes).any()), "a partial plane was left unwritten"
        runs.append(planes)
    assert torch.equal(runs[0], runs[1]), "planes differ from run to run"
    dwb.assert_untouched()
    xb.assert_untouched()
    gb.assert_untouched()
    _report("wgrad-planes" if part_shift == 0 else "wgrad-planes-unaligned", dt, *O.check(runs[0].double().sum(0), r.dw, bound), c.id)


@pytest.mark.parametrize("case_id,dt", matrix("w"))
def test_weight_gradient(case_id, dt):
    _run_wgrad(problem(case_id, dt), dt)


@pytest.mark.parametrize("case_id", ["c72_k3p1_1x17", "c24_k5p2_23x17", "c264_k3p1s2_9x12"])
def test_weight_gradient_planes_at_an_unaligned_base(case_id):
    """plane base offset by one float: the scalar-store branch of the tiled kernel's plane write (and the row kernel for comparison)"""
    _run_wgrad(problem(case_id, "bf16"), "bf16", part_shift=1)


# ------------------------------------------------------------------ what the entry points refuse
@pytest.mark.parametrize("case_id", ["c8_k3p1_66x17", "c8_k5p1s2_9x12"])
def test_fp16_gradients_are_unsupported_and_write_nothing(case_id):
    p = problem(case_id, "f16")
    c = p.case
    gb = _in_buf(c, p.dtype, p.dy).arm()
    xb = _in_buf(c, p.dtype, p.x).arm()
    ob = Buf(c.B, c.H, c.W, c.C, p.dtype).arm()
    wd = p.w.cuda()
    d = _desc(ob.t, gb.t, wd, c)
    assert _lib().dyk_dwconv_dgrad(ctypes.byref(d), None) == UNSUPPORTED
    dwb = Buf(1, 1, c.k * c.k, c.C, torch.float32, ld=c.C).arm()
    d = _desc(xb.t, gb.t, None, c)
    d.dw = dwb.t.data_ptr()
    assert _lib().dyk_dwconv_wgrad(ctypes.byref(d), None) == UNSUPPORTED
    assert _lib().dyk_dwconv_wgrad_rows(ctypes.byref(d)) == UNSUPPORTED
    torch.cuda.synchronize()
    ob.assert_untouched()
    dwb.assert_untouched()


@pytest.mark.parametrize("case_id,dt", [("c8_k2p1_6x7", "bf16"), ("c16_k4p1_9x8", "bf16"), ("c8_k2p1_6x7", "f32")])
def test_even_kernel_weight_gradient_is_unsupported_and_writes_nothing(case_id, dt):
    p = problem(case_id, dt)
    c = p.case
    xb, gb = _in_buf(c, p.dtype, p.x), _in_buf(c, p.dtype, p.dy)
    dwb = Buf(1, 1, c.k * c.k, c.C, torch.float32, ld=c.C).arm()
    d = _desc(xb.t, gb.t, None, c)
    d.dw = dwb.t.data_ptr()
    assert _lib().dyk_dwconv_wgrad(ctypes.byref(d), None) == UNSUPPORTED
    torch.cuda.synchronize()
    dwb.assert_untouched()


# ------------------------------------------------------------------ normalise + activation on load (DykDwDesc.pre)
PRE_SHAPE = (2, 72, 11, 19)         # two channel groups (the second partly filled), ragged tiles


def _pre_setup(act, k, stride):
    from dyk import ops
    B, C, H, W = PRE_SHAPE
    u, scale, shift = pre_inputs(C, B, H, W, 7)
    g = torch.Generator().manual_seed(8)
    w = (torch.randn(k * k, C, generator=g) / k).cuda()
    c = BY_ID["c72_k3p1_1x17"]._replace(id="pre", B=B, C=C, H=H, W=W, k=k, s=stride, pad=k // 2, view=False)
    Ho, Wo = out_hw(c)
    dy = torch.randn(B, C, Ho, Wo, generator=g)
    ub = Buf(B, H, W, C, torch.bfloat16, ld=C).put(u).arm()
    zb = Buf(B, H, W, C, torch.bfloat16, ld=C)
    gb = Buf(B, Ho, Wo, C, torch.bfloat16, ld=C).put(dy)
    pre = torch.stack([scale, shift]).contiguous().cuda()
    ops.call("dyk_bn_act_fwd", ops.ew_desc(a=ub.t, out=zb.t, act=act, p0=pre[0], p1=pre[1], C=C))
    torch.cuda.synchronize()
    return c, ub, zb, gb, w, pre, ops.ACT_CODES[act]


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("act", ACTS)
def test_pre_is_bit_identical_to_the_two_launch_form(act, k):
    """forward on the tiled kernel and both weight-gradient kernels (tiled at stride 1, row kernel at stride 2), planes: the same
    bits as dyk_bn_act_fwd into a stored z followed by the plain kernel.  act(shift) is ~1.5, so normalising the zero padding
    instead of padding the normalised tensor would show at every border"""
    for stride in (1, 2):
        c, ub, zb, gb, w, pre, code = _pre_setup(act, k, stride)
        Ho, Wo = out_hw(c)
        outs = []
        for src, with_pre in ((zb, False), (ub, True)):
            if stride == 1:
                yb = Buf(c.B, Ho, Wo, c.C, torch.bfloat16).arm()
                d = _desc(src.t, yb.t, w, c)
                if with_pre:
                    d.pre, d.pre_act = pre.data_ptr(), code
                _sync_ok(_lib().dyk_dwconv_fwd(ctypes.byref(d), None), "dyk_dwconv_fwd(pre)")
                yb.assert_outside_untouched()
            d = _desc(src.t, gb.t, None, c)
            dw = torch.zeros(k * k, c.C, device="cuda")
            d.dw = dw.data_ptr()
            if with_pre:
                d.pre, d.pre_act = pre.data_ptr(), code
            rows = _lib().dyk_dwconv_wgrad_rows(ctypes.byref(d))
            part = torch.full((rows, k * k, c.C), float("nan"), device="cuda")
            d.part = part.data_ptr()
            _sync_ok(_lib().dyk_dwconv_wgrad(ctypes.byref(d), None), "dyk_dwconv_wgrad(pre)")
            assert not bool(torch.isnan(part).any())
            outs.append((yb.flat.clone() if stride == 1 else None, part))
        ub.assert_untouched()
        if stride == 1:
            assert torch.equal(outs[0][0], outs[1][0]), "forward with pre differs from the two-launch form (%s, k %d)" % (act, k)
        assert torch.equal(outs[0][1], outs[1][1]), "weight gradient with pre differs from the two-launch form (%s, k %d, stride %d)" % (act, k, stride)


def test_forward_pre_off_the_tiled_kernel_is_unsupported():
    c, ub, zb, gb, w, pre, code = _pre_setup("relu", 3, 2)
    Ho, Wo = out_hw(c)
    yb = Buf(c.B, Ho, Wo, c.C, torch.bfloat16).arm()
    d = _desc(ub.t, yb.t, w, c)
    d.pre, d.pre_act = pre.data_ptr(), code
    assert _lib().dyk_dwconv_tile_ok(ctypes.byref(d)) == 0
    assert _lib().dyk_dwconv_fwd(ctypes.byref(d), None) == UNSUPPORTED
    torch.cuda.synchronize()
    yb.assert_untouched()
