"""csrc/stem.hip held to the fp64 reference of oracle/stem.py, element by element, on every dispatch path.

Every launch writes into buffers pre-filled with a sentinel: output rows of ld = Cout + 16 elements (padding channels) or tight rows,
between guard rows; statistics, dw and the partial planes between sentinel frames; images, weights and gradients framed too.
Afterwards inputs, guards and padding are bit-identical and every element in range is inside its derived bound (oracle/stem.py;
tests/test_stem_reference.py shows on the CPU that the bounds admit fp32 emulations of the kernels' arithmetic and flag eleven
kinds of wrong kernel).  The cases are those of tests/stem_cases.py.

Kernel instantiations stem.hip launches, and a case that reaches each:
  dyk_stem_conv_fwd
    stem_fwd_u8t_kernel<1 | 2, AFF, STATS, bf16>   uint8 image, 32 filters, bf16, W % 4 == 0, 4-byte-aligned image
        <S, false, true>    test_forward raw + statistics: 4x4 .. 7x520 (stride 2 at 7x520 / 6x256: the second staged word per lane;
                            stride 2 at 32 filters is the MobileNetV2 stem); 205x260x5 (two segments per workgroup across rows and images)
        <S, false, false>   test_forward raw without statistics
        <S, true, false>    test_forward, each of linear, leaky, mish, relu6, hard-swish
        <S, true, true>     test_forward affine + statistics
    stem_fwd_u8t_kernel<1 | 2, AFF, false, f16>    the same cases in f16 (raw, the five activations, the saturating store)
    stem_fwd_kernel<bf16 | float | f16, 16 | 32, U8>   everything else:
        <T, 16, true>       every uint8 case with 16 filters
        <T, 32, true>       uint8, 32 filters in f32; in bf16 / f16 at 9x47 (W % 4 != 0) and test_image_one_byte_into_its_allocation
        <T, 16 | 32, false> every float-image case; <bf16, 16, false> at 1025x512 turns the grid-stride loop
  dyk_stem_conv_wgrad
    stem_wgrad_u8_kernel<32 | 16>                  uint8 image, bf16, tight dy (lddy == Cout), W % 4 == 0, aligned: test_weight_gradient
                            `tight` at both strides (<32> at stride 2 included), test_fused_apply (bn_fused), 205x260x7 (two segments per
                            workgroup)
    stem_wgrad_kernel<bf16 | float, 16 | 32, U8>   everything else: `wide32` (lddy == 32 branch, 16 filters; also tight 32 filters in f32 or
                            with a float image), `tight` 16 filters (lddy == 16 branch), `slice` (the generic lddy branch: ld = Cout + 24),
                            uint8 at 9x47 / one byte into its allocation (U8 byte loads), test_gradient_at_a_misaligned_base,
                            205x260x7 float image in f32 (two segments per workgroup)
    stem_wgrad_fold_kernel                         every weight gradient; 205x260x7 has 2153 planes (five trips of the lane loop)

tests/test_gpu_stem.py keeps the error-code checks, the fused-against-two-pass check and the model-level uint8 check;
tests/test_gpu_fp16.py the fp16 refusal of statistics.

Every check prints `STEMRATIO <what> <dtype> <largest error / bound> <case>`; DESIGN.md ("Stem kernels against fp64") records the largest
per operation and type."""
import ctypes

import pytest
import torch

import stem_cases as SC
from oracle import stem as O
from stem_cases import SENTINEL, Buf, Flat

pytestmark = pytest.mark.gpu


def _L():
    from dyk import lib as L
    return L


def _lib():
    return _L().load()


def _desc(geo, cout, stride, dt, img):
    L = _L()
    d = L.DykStemDesc()
    d.img, d.in_u8 = img.data_ptr(), 1 if img.dtype == torch.uint8 else 0
    d.dtype = {"bf16": L.DYK_BF16, "f32": L.DYK_F32, "f16": L.DYK_F16}[dt]
    d.B, d.H, d.W, d.Cout, d.k, d.stride, d.pad = geo.B, geo.H, geo.W, cout, 3, stride, 1
    d.Ho, d.Wo = SC.out_hw(geo, stride)
    return d


def _sync_ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)
    torch.cuda.synchronize()


def _report(what, dt, ratio, bad, case):
    print("STEMRATIO %s %s %.5f %s" % (what, dt, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s %s: %d elements outside their bound, largest error / bound %.3f" % (what, dt, case, bad, ratio)


def _stats_buf(slots, C):
    st = torch.full((slots + 2, 2, C), SENTINEL, dtype=torch.float64, device="cuda")
    st[1:1 + slots] = 0
    return st


def _forward(p, u8, dt, case, tight=False, slots=0, act=None, scale=None, img_shift=0):
    """one dyk_stem_conv_fwd launch: raw (act None) or eval affine + activation, with `slots` statistics replicas"""
    geo, r, dtype = p.geo, p.ref, SC.DTYPES[dt]
    Ho, Wo = SC.out_hw(geo, p.stride)
    img = Flat(p.img8 if u8 else p.imgf, shift=img_shift).arm()
    wt = Flat(p.w.t().contiguous()).arm()
    yb = Buf(geo.B, Ho, Wo, p.cout, dtype, ld=p.cout if tight else None).arm()
    d = _desc(geo, p.cout, p.stride, dt, img.t)
    d.wt, d.y, d.ldy = wt.t.data_ptr(), yb.t.data_ptr(), yb.ld
    st = None
    if slots:
        st = _stats_buf(slots, p.cout)
        d.stats, d.stats_slots = st[1:].data_ptr(), slots
    if act is not None:
        sc = Flat(p.scale if scale is None else scale).arm()
        sh = Flat(p.shift).arm()
        d.scale, d.shift, d.act = sc.t.data_ptr(), sh.t.data_ptr(), _L().ACT_CODES[act]
    _sync_ok(_lib().dyk_stem_conv_fwd(ctypes.byref(d), None), "dyk_stem_conv_fwd")
    img.assert_untouched()
    wt.assert_untouched()
    yb.assert_outside_untouched()
    if act is None:
        what = "fwd"
        tgt, b = O.out_bound(r, dtype)
    else:
        sc.assert_untouched()
        sh.assert_untouched()
        what = "fwd-" + act if scale is None else "fwd-saturating"
        tgt, b = O.affine_bound(r, p.scale if scale is None else scale, p.shift, act, dtype)
    _report(what, dt, *O.check(yb.get(), tgt, b), case)
    if slots:
        h = st.cpu()
        assert bool((h[0] == SENTINEL).all()) and bool((h[-1] == SENTINEL).all()), "statistics written outside their slots"
        s = h[1:1 + slots].sum(0)
        b1, b2 = O.stats_bound(r)
        _report("s1", dt, *O.check(s[0], r.S1, b1), case)
        _report("s2", dt, *O.check(s[1], r.S2, b2), case)
    return yb


def _case(geo_id, cout, stride, u8, *more):
    return " ".join([geo_id, "c%d" % cout, "s%d" % stride, SC.img_kind(u8)] + [str(m) for m in more])


@pytest.mark.parametrize("geo_id,cout,stride,u8,dt", SC.forward_matrix())
def test_forward(geo_id, cout, stride, u8, dt):
    """raw with statistics at 1 and 4 slots and without; affine with each activation; affine + statistics; padded and tight rows"""
    p = SC.fwd_problem(geo_id, cout, stride)
    case = _case(geo_id, cout, stride, u8)
    stats = dt != "f16"                                 # (the inference type has no statistics epilogue: tests/test_gpu_fp16.py)
    _forward(p, u8, dt, case, tight=False, slots=1 if stats else 0)
    _forward(p, u8, dt, case, tight=True, slots=4 if stats else 0)
    if stats:
        _forward(p, u8, dt, case, tight=False)
    for i, act in enumerate(SC.ACTS):
        _forward(p, u8, dt, case, tight=bool(i & 1), act=act)
    if stats:
        _forward(p, u8, dt, case, tight=True, slots=4, act="leaky")
    else:
        big = torch.full_like(p.scale, SC.F16_OVERFLOW_SCALE)
        yb = _forward(p, u8, dt, case, act="linear", scale=big)
        assert float(yb.get().abs().max()) == O.F16_MAX, "no result saturated"


@pytest.mark.parametrize("cout,stride", [(32, 1), (32, 2), (16, 2)])
def test_forward_statistics_come_from_the_accumulators(cout, stride):
    """the constant field (tests/stem_cases.py): sums of the STORED bf16 values miss the bounds more than tenfold.  MFMA kernel (32
    filters) and scalar kernel (16)"""
    _forward(SC.const_problem(cout, stride), True, "bf16", "const c%d s%d u8" % (cout, stride), slots=1)


def test_forward_two_segments_per_workgroup():
    """205x260x5: 3075 segments over 1538 workgroups, three segments per row: the prefetch crosses rows and images"""
    geo = SC.BIG_FWD
    assert SC.mfma_forward(geo, 32, True, "bf16") and SC.segments(geo, 1) == (3, 3075) and SC.forward_segs_per_wg(geo, 1) == 2
    _forward(SC.fwd_problem(geo.id, 32, 1), True, "bf16", _case(geo.id, 32, 1, True), slots=4)


def test_scalar_forward_grid_stride_loop():
    """1025x512: 524800 pixels over 2048 workgroups of 256: 64 workgroups take a second pixel"""
    geo = SC.BIG_SCALAR
    assert not SC.mfma_forward(geo, 16, False, "bf16") and geo.B * geo.H * geo.W > 2048 * 256
    _forward(SC.fwd_problem(geo.id, 16, 1), False, "bf16", _case(geo.id, 16, 1, False), slots=4)


# ---------------------------------------------------------------------------------------------------- weight gradient
def _wgrad(p, dt, layout, case, img_shift=0, dy_shift=0):
    """dyk_stem_conv_wgrad twice onto the same non-zero dw: inside the bound, bit-identical, planes fully written"""
    geo, cout = p.geo, p.cout
    Ho, Wo = SC.out_hw(geo, p.stride)
    lddy, off = SC.dy_layout(cout, layout)
    img = Flat(p.img, shift=img_shift).arm()
    gb = Buf(geo.B, Ho, Wo, cout, p.dtype, ld=lddy, off=off, shift=dy_shift).put(p.dy).arm()
    d = _desc(geo, cout, p.stride, dt, img.t)
    d.dy, d.lddy = gb.t.data_ptr(), lddy
    planes = _lib().dyk_stem_wgrad_planes(ctypes.byref(d))
    assert planes == SC.wgrad_planes(geo, p.stride)[1]
    sum_then_scale = SC.u8_wgrad(geo, cout, p.u8, dt, lddy, aligned=img_shift == 0 and dy_shift == 0)
    runs = []
    for _ in range(2):
        dw = Flat(p.old).arm()
        part = Flat(torch.empty(planes * cout * 27), fill=float("nan")).arm()
        d.dw, d.part = dw.t.data_ptr(), part.t.data_ptr()
        _sync_ok(_lib().dyk_stem_conv_wgrad(ctypes.byref(d), None), "dyk_stem_conv_wgrad")
        dw.assert_outside_untouched()
        part.assert_outside_untouched()
        assert not bool(torch.isnan(part.t).any()), "a partial plane was left unwritten"
        runs.append((dw.t.cpu(), part.t.cpu()))
    img.assert_untouched()
    gb.assert_untouched()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "weight gradient differs from run to run"
    what = "wgrad-%s%s" % (p.field, "-sum-then-scale" if sum_then_scale else "")
    _report(what, dt, *O.check(runs[0][0], *SC.wgrad_bound(p, sum_then_scale)), case)


@pytest.mark.parametrize("geo_id,cout,stride,u8,dt,layout", SC.wgrad_matrix())
def test_weight_gradient(geo_id, cout, stride, u8, dt, layout):
    case = _case(geo_id, cout, stride, u8, layout)
    _wgrad(SC.wgrad_problem(geo_id, cout, stride, u8, dt, "exact"), dt, layout, case)
    p = SC.wgrad_problem(geo_id, cout, stride, u8, dt, "random")
    if p.n <= 2048:
        _wgrad(p, dt, layout, case)


@pytest.mark.parametrize("cout,u8,dt", [(32, True, "bf16"), (16, True, "bf16"), (32, False, "f32")])
def test_weight_gradient_two_segments_per_workgroup(cout, u8, dt):
    """205x260x7 on the exact field: 4305 segments over 2153 workgroups and planes; the uint8 MFMA kernel at 32 and 16 filters, the generic
    kernel with a float p / 256 image in fp32 (lddy 32)"""
    geo = SC.BIG_WGRAD
    assert SC.segments(geo, 1)[1] == 4305 and SC.wgrad_planes(geo, 1) == (2, 2153)
    assert SC.u8_wgrad(geo, cout, u8, dt, cout) == u8
    _wgrad(SC.wgrad_problem(geo.id, cout, 1, u8, dt, "exact", False), dt, "tight", _case(geo.id, cout, 1, u8, "tight"))


# ---------------------------------------------------------------------------------------------------- misaligned bases
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("geo_id", ["4x4", "3x128", "7x520"])
def test_image_one_byte_into_its_allocation(geo_id, stride):
    """W % 4 == 0 but img % 4 == 1: the word-load kernels must not run; the scalar forward and the byte-load weight gradient give the
    same values"""
    geo = SC.BY_ID[geo_id]
    assert geo.W % 4 == 0 and not SC.mfma_forward(geo, 32, True, "bf16", aligned=False)
    p = SC.fwd_problem(geo_id, 32, stride)
    case = _case(geo_id, 32, stride, True, "img+1")
    _forward(p, True, "bf16", case, slots=4, img_shift=1)
    _forward(p, True, "f16", case, act="mish", img_shift=1)
    for cout in (32, 16):
        q = SC.wgrad_problem(geo_id, cout, stride, True, "bf16", "exact")
        _wgrad(q, "bf16", "tight", _case(geo_id, cout, stride, True, "tight img+1"), img_shift=1)


@pytest.mark.parametrize("cout,u8,dt", [(32, True, "bf16"), (16, True, "bf16"), (16, False, "f32"), (32, False, "f32")])
@pytest.mark.parametrize("geo_id,stride", [("5x132", 1), ("7x520", 2)])
def test_gradient_at_a_misaligned_base(geo_id, stride, cout, u8, dt):
    """dy 8 bytes off a 16-byte boundary, tight rows: the uint8 MFMA kernel and the 16-byte branch of the tight 16-filter staging must not run"""
    p = SC.wgrad_problem(geo_id, cout, stride, u8, dt, "exact")
    shift = 8 // (2 if dt == "bf16" else 4)
    _wgrad(p, dt, "tight", _case(geo_id, cout, stride, u8, "tight dy+8B"), dy_shift=shift)


# ---------------------------------------------------------------------------------------------------- fused BatchNorm-backward apply
@pytest.mark.parametrize("slots", SC.FUSED_SLOTS)
@pytest.mark.parametrize("geo_id,cout,stride", SC.FUSED)
def test_fused_apply(geo_id, cout, stride, slots):
    """DykStemDesc.bn_fused: dw += sum bf16(dz) patch with dz = scale (da - S1/N - xhat S2/N) applied on load, dgamma += S2, dbeta += S1"""
    p = SC.fused_problem(geo_id, cout, stride)
    geo = p.geo
    Ho, Wo = SC.out_hw(geo, stride)
    red_h = SC.fused_red(p, slots)
    f = SC.fused_ref(p, red_h)
    assert f.share <= O.AMBIGUOUS_SHARE
    case = _case(geo_id, cout, stride, True, "slots %d" % slots)
    img = Flat(p.img8).arm()
    da = Buf(geo.B, Ho, Wo, cout, torch.bfloat16, ld=cout).put(p.da).arm()
    yraw = Buf(geo.B, Ho, Wo, cout, torch.bfloat16, ld=cout).put(p.yraw).arm()
    vecs = Flat(torch.cat([p.scale, torch.zeros(cout), p.mean, p.rstd])).arm()
    red = Flat(red_h).arm()
    dg, db, dw = Flat(p.old_dg).arm(), Flat(p.old_db).arm(), Flat(p.old_dw).arm()
    d = _desc(geo, cout, stride, "bf16", img.t)
    d.lddy = cout
    planes = _lib().dyk_stem_wgrad_planes(ctypes.byref(d))
    part = Flat(torch.empty(planes * cout * 27), fill=float("nan")).arm()
    d.dw, d.part = dw.t.data_ptr(), part.t.data_ptr()
    d.bn_da, d.bn_yraw, d.bn_vecs, d.bn_red, d.bn_slots = da.t.data_ptr(), yraw.t.data_ptr(), vecs.t.data_ptr(), red.t.data_ptr(), slots
    d.bn_dgamma, d.bn_dbeta = dg.t.data_ptr(), db.t.data_ptr()
    assert _lib().dyk_stem_wgrad_bn_fusable(ctypes.byref(d)) == 1
    d.bn_fused = 1
    _sync_ok(_lib().dyk_stem_conv_wgrad(ctypes.byref(d), None), "dyk_stem_conv_wgrad(bn_fused)")
    for b in (img, da, yraw, vecs, red):
        b.assert_untouched()
    for b in (dg, db, dw, part):
        b.assert_outside_untouched()
    assert not bool(torch.isnan(part.t).any()), "a partial plane was left unwritten"
    _report("fused-dw", "bf16", *O.check(dw.t.cpu(), *O.fused_dw_bound(f, p.P, p.n, p.old_dw)), case)
    _report("fused-dgamma", "bf16", *O.check(dg.t.cpu(), *O.sum_bound(f.S2, p.old_dg)), case)
    _report("fused-dbeta", "bf16", *O.check(db.t.cpu(), *O.sum_bound(f.S1, p.old_db)), case)
