"""csrc/elementwise.hip held to the fp64 reference of oracle/elementwise.py, element by element, on every dispatch path.

Every launch reads and writes sentinel-framed buffers (tests/elementwise_cases.py): channels-last rows either tight or as the slice
[8 : 8 + C] of rows of C + 24 elements, between guard rows; argmax, pooled, the workspaces, red and the scratch between sentinel frames.
Afterwards inputs, guards and padding channels are bit-identical and every element in range equals its reference (pool values and codes,
copies, the permutes: bit for bit) or lies inside its derived bound (tests/test_elementwise_reference.py shows on the CPU that the bounds
admit fp32 emulations of the kernels' arithmetic and flag each of a list of wrong kernels).

Kernel instantiations elementwise.hip launches, and a case that reaches each:
  dyk_maxpool_fwd
    maxpool_tile_fwd_kernel<bf16 | float | f16>    test_tile_pool: maps 1x1 .. 32x32 (1024 threads, 40960 bytes of LDS), k 1 .. 15, with and without argmax
    maxpool_fwd_kernel<T, 3 | 5 | 9 | 13>          test_generic_pool_stride_1 (33x32: 1056 pixels); <T, 2 | 3 | 5 | 9 | 13> also test_strided_pool
    maxpool_fwd_kernel<T, 0>                       test_generic_pool_stride_1 k = 7, 15; test_strided_pool (4,1), (15,8)
    maxpool_fwd_kernel<bf16, 3> grid-stride loop   test_pool_grid_stride_loop (1025x1024)
  dyk_maxpool_bwd
    maxpool_tile_bwd_kernel<bf16 | float>          test_tile_pool: store, accumulate, NaN gradients; 32x32: 65536 bytes of LDS, 1024 threads
    maxpool_bwd_kernel<bf16 | float, K>            the generic and strided tests, K as above; the grid-stride case
  dyk_upsample2x_fwd   upsample2x_fwd_kernel<bf16 | float | f16>   test_upsample; loop: test_upsample_grid_stride_loops
  dyk_upsample2x_bwd   upsample2x_bwd_kernel<bf16 | float>         test_upsample; loop: test_upsample_grid_stride_loops
  dyk_axpby            axpby_kernel<bf16 | float | f16>            test_axpby_forms (every operand combination), test_axpby_twin_launch
                                                                   (gridDim.z = 2), test_axpby_and_dot_grid_stride_loops
  dyk_dot              dot_kernel<bf16 | float>                    test_dot; the 1024-workgroup cap: test_axpby_and_dot_grid_stride_loops
  dyk_wfuse_weights, dyk_wfuse_bwd_params   wfuse_weights_kernel, wfuse_bwd_params_kernel   test_weighted_fusion_weights (n = 1 .. 64)
  dyk_se_pool          se_pool_kernel<bf16 | float | f16>, se_pool_fold_kernel   test_se_pool (CVB 1 / 4 / 16, HS 1 / 2 / 16, ragged last chunk)
  dyk_se_fc_fwd        se_rows_kernel<0 | 1>                       test_se_fc_forward: bper 1, 2, 3 (last slice short); dot16 at K = 4, 8, 16, 64,
                                                                   132, 240, 260, 960, 8192 (every mask of the second to fourth loads)
  dyk_se_fc_bwd        se_cols_kernel<0 | 1>, se_fc_wgrad_kernel   test_se_fc_backward: data half, parameter half, both; C = 8192, B = 256
  dyk_se_scale         se_scale_kernel<bf16 | float | f16, -2>     test_se_scale
                       se_scale_kernel<bf16 | float, MISH | RELU | HSWISH | RELU6 | -1>   test_se_scale_with_the_batchnorm_backward_reduce;
                                                                   the image loop: test_se_scale_reduce_walks_several_images
  dyk_head_permute_fwd head_permute_fwd_kernel                     test_head
  dyk_head_permute_bwd head_permute_bwd_kernel<float | bf16>, head_bias_grad_kernel   test_head (the four-load loop at 3073, 4097 and 5120 cells)

tests/test_gpu_elementwise.py keeps the error-code and module-level checks.

Every check prints `EWRATIO <op> <dtype> <largest error / bound> <case>` (0 for the bit-for-bit ones); DESIGN.md ("Elementwise kernels
against fp64") records the largest per operation and type."""
import ctypes

import pytest
import torch

import elementwise_cases as EC
from elementwise_cases import Flat
from oracle import elementwise as O

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _L():
    from dyk import lib as L
    return L


def _lib():
    return _L().load()


def _ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)
    torch.cuda.synchronize()


def _report(op, dt, ratio, bad, case):
    print("EWRATIO %s %s %.5f %s" % (op, dt, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s %s: %d elements outside their bound, largest error / bound %.3f" % (op, dt, case, bad, ratio)


def _exact(op, dt, got, want, case):
    """bit for bit"""
    bad = O.same_bits(got, want)
    print("EWRATIO %s %s %.5f %s" % (op, dt, 0.0, case))
    assert bad == 0, "%s %s %s: %d elements differ from the reference" % (op, dt, case, bad)


def _ptr(t):
    return None if t is None else (t.t.data_ptr() if hasattr(t, "t") else t.data_ptr())


def _desc(dt, C, a=None, b=None, out=None, **kw):
    """a DykEwDesc over Bufs (a, b, out) and tensors / Flats / numbers (the rest)"""
    L = _L()
    d = L.DykEwDesc()
    d.dtype = {"bf16": L.DYK_BF16, "f32": L.DYK_F32, "f16": L.DYK_F16}[dt]
    d.C, d.alpha, d.beta = C, 1.0, 1.0
    for nm, buf, ldn in (("a", a, "lda"), ("b", b, "ldb"), ("out", out, "ldo")):
        if buf is not None:
            setattr(d, nm, buf.t.data_ptr())
            setattr(d, ldn, buf.ld)
    for k, v in kw.items():
        setattr(d, k, v if isinstance(v, (int, float)) or v is None else _ptr(v))
    return d


def _nchw(buf):
    """the Buf's elements as a float32 NCHW tensor on the host (exact for every storage type)"""
    return buf.t.cpu().permute(0, 3, 1, 2).float()


def _to_rows(x, dt):
    """NCHW float -> NHWC of the storage type"""
    return x.permute(0, 2, 3, 1).contiguous().to(EC.DTYPES[dt])


def _other(lay):
    return "slice" if lay == "tight" else "tight"


# ---------------------------------------------------------------------------------------------------- max pool
def _pool_forward(dt, B, C, H, W, k, stride, lay, case, argmax=True):
    x = EC.pool_input(B, C, H, W)
    vals, codes = EC.pool_ref(B, C, H, W, k, stride)
    Ho, Wo = codes.shape[2:]
    xin = EC.nhwc(x, dt, lay)
    out = EC.nhwc(vals, dt, _other(lay), fill=False)
    am = Flat(torch.zeros(B, Ho, Wo, C, dtype=torch.uint8), fill=255).arm() if argmax else None
    d = _desc(dt, C, a=xin, out=out, B=B, H=H, W=W, k=k, slots=stride)
    _ok(_lib().dyk_maxpool_fwd(ctypes.byref(d), _ptr(am), None), "dyk_maxpool_fwd")
    xin.assert_untouched()
    out.assert_outside_untouched()
    # (the values are elements of the input, so the type's store rule is exact on them -- but for fp16's, which saturates: +-inf leaves as
    # +-65504, as from every other fp16 store of the library, tests/test_gpu_fp16.py)
    want = O.store(vals, EC.DTYPES[dt]).permute(0, 2, 3, 1).contiguous()
    _exact("pool-fwd" if argmax else "pool-fwd-noargmax", dt, out.t.cpu(), want, case)
    if argmax:
        am.assert_outside_untouched()
        _exact("pool-codes", dt, am.t.cpu(), codes.permute(0, 2, 3, 1).contiguous(), case)


def _pool_backward(dt, B, C, H, W, k, stride, lay, case, accumulate=False, nan=False):
    dy, old, tgt, bound = EC.pool_bwd_ref(B, C, H, W, k, stride, dt, nan, accumulate)
    codes = EC.pool_ref(B, C, H, W, k, stride)[1]
    g = EC.nhwc(dy, dt, lay)
    am = Flat(codes.permute(0, 2, 3, 1).contiguous()).arm()
    out = EC.nhwc(tgt if old is None else old, dt, _other(lay), fill=old is not None)
    d = _desc(dt, C, a=g, out=out, B=B, H=H, W=W, k=k, slots=stride, flags=_L().EW_ACCUM if accumulate else 0)
    _ok(_lib().dyk_maxpool_bwd(ctypes.byref(d), _ptr(am), None), "dyk_maxpool_bwd")
    g.assert_untouched()
    am.assert_untouched()
    out.assert_outside_untouched()
    op = "pool-bwd" + ("-accum" if accumulate else "") + ("-nan" if nan else "")
    _report(op, dt, *O.check_nan(_nchw(out), tgt, bound), case)


def _pool_all(dt, B, C, H, W, k, stride, lay, case, full=True):
    _pool_forward(dt, B, C, H, W, k, stride, lay, case)
    if full:
        _pool_forward(dt, B, C, H, W, k, stride, _other(lay), case, argmax=False)
    if dt == "f16":
        return
    _pool_backward(dt, B, C, H, W, k, stride, lay, case)
    if full:
        _pool_backward(dt, B, C, H, W, k, stride, _other(lay), case, accumulate=True)
        _pool_backward(dt, B, C, H, W, k, stride, lay, case, nan=True)


@pytest.mark.parametrize("H,W,k", EC.tile_matrix())
def test_tile_pool(H, W, k):
    """the LDS-plane kernels: values and codes bit for bit with and without argmax; backward store, accumulate and with NaN gradients"""
    for dt, C, B, lay in EC.tile_variants(H, W, k):
        _pool_all(dt, B, C, H, W, k, 1, lay, "tile %dx%d k%d c%d b%d %s" % (H, W, k, C, B, lay))


@pytest.mark.parametrize("k", EC.GENERIC_KS)
def test_generic_pool_stride_1(k):
    """33x32 = 1056 pixels: past the tile limit, the generic kernels at stride 1 (what the SPP block runs on large images)"""
    H, W = EC.GENERIC_MAP
    for dt, C, lay in (("bf16", 8, "tight"), ("f32", 4, "slice"), ("f16", 8, "slice"), ("bf16", 24, "slice")):
        assert not EC.tile_ok(k, 1, H, W, C) and EC.pool_K(k) == (k if k in (3, 5, 9, 13) else 0)
        _pool_all(dt, 1, C, H, W, k, 1, lay, "generic %dx%d k%d c%d %s" % (H, W, k, C, lay))


@pytest.mark.parametrize("H,W", EC.STRIDED_MAPS)
@pytest.mark.parametrize("k,stride", EC.STRIDED)
def test_strided_pool(k, stride, H, W):
    """nn.MaxPool2d(k, stride, (k - 1) // 2) on odd maps (the last window is clipped) and on maps smaller than the window.  A map with
    no output (an even window on one pixel) is refused where the package sizes a pool's output (dyk.ops.maxpool_out_size, as torch
    refuses it), before anything is allocated or launched: the kernels would make it one output at stride 2"""
    Ho, Wo = EC.pool_shape(H, W, k, stride)
    if Ho == 0 or Wo == 0:
        from dyk import functional as Fn
        with pytest.raises(ValueError):
            Fn.maxpool(torch.zeros(2, 8, H, W, device="cuda"), k, stride)
        return
    for dt, C, lay in (("bf16", 8, "slice"), ("f32", 4, "tight"), ("f16", 16, "tight")):
        case = "strided %dx%d k%d s%d c%d %s" % (H, W, k, stride, C, lay)
        assert not EC.tile_ok(k, stride, H, W, C)
        _pool_all(dt, 2, C, H, W, k, stride, lay, case)


def test_pool_grid_stride_loop():
    """1025x1024, C = 8, bf16, k = 3: 1049600 vectors over 4096 workgroups of 256: 1024 threads take a second vector, forward and backward"""
    H, W = EC.BIG_POOL
    assert not EC.tile_ok(3, 1, H, W, 8) and H * W * (8 // EC.epv("bf16")) > EC.EW_CAP
    _pool_all("bf16", 1, 8, H, W, 3, 1, "tight", "generic 1025x1024 k3 c8 tight", full=False)


# ---------------------------------------------------------------------------------------------------- upsample
def _upsample(dt, B, C, H, W, lay, case, backward=True):
    x = EC.rand_tensor(B, C, H, W, dt, 1)
    xin = EC.nhwc(x, dt, lay)
    up = O.up_fwd(x)
    out = EC.nhwc(up, dt, _other(lay), fill=False)
    d = _desc(dt, C, a=xin, out=out, B=B, H=H, W=W)
    _ok(_lib().dyk_upsample2x_fwd(ctypes.byref(d), None), "dyk_upsample2x_fwd")
    xin.assert_untouched()
    out.assert_outside_untouched()
    _exact("up-fwd", dt, out.t.cpu(), _to_rows(up, dt), case)
    if dt == "f16" or not backward:
        return
    _upsample_bwd(dt, B, C, H, W, lay, case, False)
    _upsample_bwd(dt, B, C, H, W, _other(lay), case, True)


def _upsample_bwd(dt, B, C, H, W, lay, case, accumulate):
    g = EC.rand_tensor(B, C, 2 * H, 2 * W, dt, 2)
    old = EC.rand_tensor(B, C, H, W, dt, 3) if accumulate else None
    tgt, bound = O.up_bwd(g, EC.DTYPES[dt], old)
    gin = EC.nhwc(g, dt, lay)
    out = EC.nhwc(tgt if old is None else old, dt, _other(lay), fill=accumulate)
    d = _desc(dt, C, a=gin, out=out, B=B, H=H, W=W, flags=_L().EW_ACCUM if accumulate else 0)
    _ok(_lib().dyk_upsample2x_bwd(ctypes.byref(d), None), "dyk_upsample2x_bwd")
    gin.assert_untouched()
    out.assert_outside_untouched()
    _report("up-bwd" + ("-accum" if accumulate else ""), dt, *O.check(_nchw(out), tgt, bound), case)


@pytest.mark.parametrize("C", EC.UP_C)
@pytest.mark.parametrize("H,W", EC.UP_MAPS)
def test_upsample(H, W, C):
    for dt, c in (("bf16", C), ("f32", C // 2), ("f16", C)):
        for lay in ("tight", "slice"):
            _upsample(dt, 2, c, H, W, lay, "up %dx%d c%d %s" % (H, W, c, lay))


def test_upsample_grid_stride_loops():
    """forward from a 513x512 map (1050624 output vectors) and backward onto a 1025x1024 map (1049600 vectors), C = 8, bf16"""
    H, W = EC.BIG_UP_FWD
    assert 4 * H * W > EC.EW_CAP
    _upsample("bf16", 1, 8, H, W, "tight", "up 513x512 c8", backward=False)
    H, W = EC.BIG_UP_BWD
    assert H * W > EC.EW_CAP
    _upsample_bwd("bf16", 1, 8, H, W, "tight", "up-bwd 1025x1024 c8", False)


# ---------------------------------------------------------------------------------------------------- axpby / dot
ALPHA, BETA, P0, P1 = 0.75, -1.25, 1.5, 0.3


def _axpby(dt, B, C, H, W, form, lays, case, alpha=ALPHA, a_nan=False):
    """one launch; returns (out Buf, target, bound)"""
    has_b, has_p0, has_p1, accumulate, in_place = form
    la, lb, lo = lays
    a = EC.rand_tensor(B, C, H, W, dt, 11)
    b = EC.rand_tensor(B, C, H, W, dt, 12) if has_b else None
    old = a if in_place else EC.rand_tensor(B, C, H, W, dt, 13)
    a_dev = torch.full_like(a, NAN) if a_nan else a
    abuf = EC.nhwc(a_dev, dt, la)
    bbuf = EC.nhwc(b, dt, lb) if has_b else None
    obuf = abuf if in_place else EC.nhwc(old, dt, lo, fill=accumulate)
    p0 = Flat(torch.tensor([P0])).arm() if has_p0 else None
    p1 = Flat(torch.tensor([P1])).arm() if has_p1 else None
    d = _desc(dt, C, a=abuf, b=bbuf, out=obuf, npix=B * H * W, alpha=alpha, beta=BETA, p0=p0, p1=p1,
              flags=_L().EW_ACCUM if accumulate else 0)
    _ok(_lib().dyk_axpby(ctypes.byref(d), None), "dyk_axpby")
    if not in_place:
        abuf.assert_untouched()
    for f in (bbuf, p0, p1):
        if f is not None:
            f.assert_untouched()
    obuf.assert_outside_untouched()
    tgt, bound = O.axpby(a, EC.DTYPES[dt], alpha, BETA, b, P0 if has_p0 else None, P1 if has_p1 else None, old if accumulate else None)
    _report("axpby", dt, *O.check(_nchw(obuf), tgt, bound), case)
    return obuf


@pytest.mark.parametrize("lays", EC.AXPBY_LDS, ids=lambda l: "-".join(l))
@pytest.mark.parametrize("dt,C", [("bf16", 24), ("f32", 12), ("f16", 8)])
def test_axpby_forms(dt, C, lays):
    """b, p0, p1 present or not, accumulate, in place; alpha = 0 over a NaN buffer clears or passes b / old through"""
    for form in EC.AXPBY_FORMS:
        if form[4] and lays[0] != lays[2]:
            continue                                                        # (in place: one buffer, one layout)
        _axpby(dt, 2, C, 3, 5, form, lays, "axpby c%d %s b%d p0%d p1%d acc%d inplace%d" % ((C, "-".join(lays)) + tuple(map(int, form))))
    for form in ((False, False, False, False, False), (True, True, True, False, False), (False, False, False, False, True)):
        _axpby(dt, 2, C, 3, 5, form, (lays[0], lays[1], lays[0] if form[4] else lays[2]), "axpby alpha=0 over NaN c%d" % C, alpha=0.0,
               a_nan=True)


@pytest.mark.parametrize("dt,C", [("bf16", 24), ("f32", 12)])
def test_axpby_twin_launch(dt, C):
    """two problems in one launch (DykEwDesc.twin, gridDim.z = 2) give the bits of two single launches"""
    B, H, W = 2, 3, 5
    x = [EC.rand_tensor(B, C, H, W, dt, 20 + i) for i in range(4)]
    ins = [EC.nhwc(t, dt, "slice") for t in x]
    p = [Flat(torch.tensor([v])).arm() for v in (P0, P1, -0.6, 2.25)]
    single = [EC.nhwc(x[0], dt, "slice", fill=False) for _ in range(2)]
    twin = [EC.nhwc(x[0], dt, "slice", fill=False) for _ in range(2)]

    def descs(outs):
        return [_desc(dt, C, a=ins[2 * i], b=ins[2 * i + 1], out=outs[i], npix=B * H * W, alpha=ALPHA, beta=BETA, p0=p[2 * i], p1=p[2 * i + 1])
                for i in range(2)]
    for d in descs(single):
        _ok(_lib().dyk_axpby(ctypes.byref(d), None), "dyk_axpby")
    d0, d1 = descs(twin)
    d0.twin = ctypes.addressof(d1)
    _ok(_lib().dyk_axpby(ctypes.byref(d0), None), "dyk_axpby(twin)")
    for i in range(2):
        twin[i].assert_outside_untouched()
        _exact("axpby-twin", dt, twin[i].t.cpu(), single[i].t.cpu(), "twin problem %d c%d" % (i, C))
        tgt, bound = O.axpby(x[2 * i], EC.DTYPES[dt], ALPHA, BETA, x[2 * i + 1], (P0, -0.6)[i], (P1, 2.25)[i])
        _report("axpby", dt, *O.check(_nchw(twin[i]), tgt, bound), "twin problem %d c%d" % (i, C))
    for f in ins + p:
        f.assert_untouched()


def _dot(dt, B, C, H, W, lays, case, with_out=None, old_red=0.375):
    """with_out: None, "store" or "accum" (the scaled copy of `a` the same pass leaves)"""
    a, b = EC.rand_tensor(B, C, H, W, dt, 31), EC.rand_tensor(B, C, H, W, dt, 32)
    abuf, bbuf = EC.nhwc(a, dt, lays[0]), EC.nhwc(b, dt, lays[1])
    red = Flat(torch.tensor([7.0, old_red, 7.0], dtype=torch.float64)).arm()
    obuf = p0 = old = None
    if with_out:
        old = EC.rand_tensor(B, C, H, W, dt, 33)
        obuf = EC.nhwc(old, dt, lays[2], fill=with_out == "accum")
        p0 = Flat(torch.tensor([P0])).arm()
    d = _desc(dt, C, a=abuf, b=bbuf, out=obuf, npix=B * H * W, alpha=ALPHA, p0=p0, flags=_L().EW_ACCUM if with_out == "accum" else 0)
    d.red = red.t[1:].data_ptr()
    _ok(_lib().dyk_dot(ctypes.byref(d), None), "dyk_dot")
    abuf.assert_untouched()
    bbuf.assert_untouched()
    red.assert_outside_untouched()
    r = red.t.cpu()
    assert float(r[0]) == 7.0 and float(r[2]) == 7.0, "red written beside its element"
    vecs = B * H * W * (C // EC.epv(dt))
    s, bound = O.dot(a, b, EC.epv(dt), EC.dot_trips(vecs), EC.dot_grid(vecs))
    tgt = s + old_red
    _report("dot", dt, *O.check(r[1:2], tgt.view(1), torch.tensor([bound + O.U64 * abs(float(tgt))])), case)
    if with_out:
        p0.assert_untouched()
        obuf.assert_outside_untouched()
        tgt, bound = O.axpby(a, EC.DTYPES[dt], ALPHA, 1.0, None, P0, None, old if with_out == "accum" else None)
        _report("dot-out", dt, *O.check(_nchw(obuf), tgt, bound), case)


@pytest.mark.parametrize("dt,C", [("bf16", 24), ("f32", 12)])
def test_dot(dt, C):
    for lays in EC.AXPBY_LDS:
        for with_out in (None, "store", "accum"):
            _dot(dt, 2, C, 3, 5, lays, "dot c%d %s out=%s" % (C, "-".join(lays), with_out), with_out)


def test_axpby_and_dot_grid_stride_loops():
    """axpby over 1049600 vectors (4096-workgroup cap) and dot over 2099200 (1024-workgroup cap: nine trips for some threads), C = 8, bf16"""
    H, W = EC.BIG_AXPBY
    assert H * W > EC.EW_CAP
    _axpby("bf16", 1, 8, H, W, (True, True, True, True, False), ("tight", "tight", "tight"), "axpby 1025x1024 c8")
    H, W = EC.BIG_DOT
    assert H * W > 1024 * 2048 and EC.dot_grid(H * W) == 1024 and EC.dot_trips(H * W) == 9
    _dot("bf16", 1, 8, H, W, ("tight", "tight", "tight"), "dot 1025x2048 c8", "store")


@pytest.mark.parametrize("n", EC.WFUSE_N)
def test_weighted_fusion_weights(n):
    """weff = sigmoid(w) * 2 / n and dw += red * 2 / n * s * (1 - s) over w in [-12, 12], inside the bound built on the measured __expf
    figure (oracle/elementwise.py); lanes >= n write nothing"""
    w, red, old = EC.wfuse_problem(n)
    wf, rf = Flat(w).arm(), Flat(red).arm()
    weff = Flat(torch.zeros(n), fill=NAN).arm()
    dw = Flat(old).arm()
    _ok(_lib().dyk_wfuse_weights(_ptr(wf), _ptr(weff), n, None), "dyk_wfuse_weights")
    _ok(_lib().dyk_wfuse_bwd_params(_ptr(wf), _ptr(rf), _ptr(dw), n, None), "dyk_wfuse_bwd_params")
    wf.assert_untouched()
    rf.assert_untouched()
    weff.assert_outside_untouched()
    dw.assert_outside_untouched()
    _report("wfuse-weights", "f32", *O.check(weff.t.cpu(), *O.wfuse_weights(w)), "n=%d" % n)
    _report("wfuse-bwd", "f32", *O.check(dw.t.cpu(), *O.wfuse_bwd(w, red, old)), "n=%d" % n)


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
@pytest.mark.parametrize("H,W", EC.SE_POOL_MAPS)
@pytest.mark.parametrize("dt,C", EC.SE_POOL_C + [("f16", 8)])
def test_se_pool(dt, C, H, W):
    """with and without the second operand, with and without the scratch; the split path shows in the NaN-filled scratch: exactly
    HS * B * C floats of it are written when HS > 1, none otherwise"""
    L = _L()
    B, HW = 2, H * W
    x, y = EC.rand_tensor(B, C, H, W, dt, 41), EC.rand_tensor(B, C, H, W, dt, 42)
    for i, (second, scratch) in enumerate(((False, False), (False, True), (True, True), (True, False))):
        CVB, PY, gx, HS, chunk = EC.se_pool_geo(C, dt, B, HW, scratch)
        want = EC.SE_POOL_PATHS.get((dt, C, (H, W), scratch))
        assert want is None or want == (CVB, HS)
        case = "se_pool %dx%d c%d b=%d scratch=%d CVB%d HS%d" % (H, W, C, second, scratch, CVB, HS)
        lay = ("tight", "slice")[i % 2]
        xb = EC.nhwc(x, dt, lay)
        yb = EC.nhwc(y, dt, _other(lay)) if second else None
        pooled = Flat(torch.zeros(B, C), fill=NAN).arm()
        sc = Flat(torch.zeros(L.SE_POOL_SPLITS * B * C), fill=NAN).arm()
        alpha = 0.5 if second else 1.0 / HW
        d = _desc(dt, C, a=xb, b=yb, B=B, H=H, W=W, alpha=alpha, aux2=sc if scratch else None)
        _ok(_lib().dyk_se_pool(ctypes.byref(d), _ptr(pooled), None), "dyk_se_pool")
        xb.assert_untouched()
        if second:
            yb.assert_untouched()
        pooled.assert_outside_untouched()
        sc.assert_outside_untouched()
        written = int((~torch.isnan(sc.t)).sum())
        assert written == (HS * B * C if HS > 1 else 0), "%s: %d scratch floats written" % (case, written)
        tgt, bound = O.se_pool(x, alpha, EC.se_pool_m(C, dt, B, HW, scratch), y if second else None)
        _report("se_pool" + ("-xy" if second else ""), dt, *O.check(pooled.t.cpu(), tgt, bound), case)


def _se_desc(p, bufs):
    d = _L().DykSeFcDesc()
    d.B, d.C, d.Cs = p.B, p.C, p.Cs
    for k, v in bufs.items():
        setattr(d, k, _ptr(v))
    return d


def _se_inputs(p):
    return {k: Flat(getattr(p, k)).arm() for k in ("pooled", "w1", "b1", "w2", "b2")}


@pytest.mark.parametrize("C,Cs,B", EC.SE_FC)
def test_se_fc_forward(C, Cs, B):
    """h against pooled; t2 and scale against the h the device stored; dt1's part of the workspace stays as it was"""
    p = EC.se_problem(C, Cs, B)
    bper = EC.se_rows_grid(C, B)[2]
    assert EC.SE_FC_BPER.get((C, Cs, B), bper) == bper and (bper > 1) == (-(-C // 16) * B > 512)
    case = "se_fc c%d cs%d b%d bper%d" % (C, Cs, B, bper)
    ins = _se_inputs(p)
    scale = Flat(torch.zeros(B, C), fill=NAN).arm()
    ws = Flat(torch.zeros(B * (C + 2 * Cs)), fill=NAN).arm()
    d = _se_desc(p, dict(ins, scale=scale, ws=ws))
    _ok(_lib().dyk_se_fc_fwd(ctypes.byref(d), None), "dyk_se_fc_fwd")
    for f in ins.values():
        f.assert_untouched()
    scale.assert_outside_untouched()
    ws.assert_outside_untouched()
    w = ws.t.cpu()
    h, dt1, t2 = w[:B * Cs].view(B, Cs), w[B * Cs:2 * B * Cs], w[2 * B * Cs:].view(B, C)
    assert bool(torch.isnan(dt1).all()), "the forward call wrote into dt1"
    _report("se_fc-h", "f32", *O.check(h, *O.se_fc1(p.pooled, p.w1, p.b1)), case)
    (t_ref, t_b), (s_ref, s_b) = O.se_fc2(h, p.w2, p.b2)
    _report("se_fc-t2", "f32", *O.check(t2, t_ref, t_b), case)
    _report("se_fc-scale", "f32", *O.check(scale.t.cpu(), s_ref, s_b), case)


@pytest.mark.parametrize("half", ["data", "params", "both"])
@pytest.mark.parametrize("C,Cs,B", EC.SE_FC)
def test_se_fc_backward(C, Cs, B, half):
    """a workspace the test writes: t2 with exact +-3, h with exact zeros.  data half: dt1 and dpooled (against the dt1 the device stored);
    parameter half: the four gradients on top of non-zero contents, nothing else written"""
    p = EC.se_problem(C, Cs, B)
    case = "se_fc c%d cs%d b%d %s" % (C, Cs, B, half)
    data, params = half != "params", half != "data"
    ins = _se_inputs(p)
    ins["dscale"] = Flat(p.dscale).arm()
    dt1_in = torch.full_like(p.dt1, NAN) if data else p.dt1
    ws = Flat(torch.cat([p.h.reshape(-1), dt1_in.reshape(-1), p.t2.reshape(-1)])).arm()
    bufs = dict(ins, ws=ws)
    if data:
        bufs["dpooled"] = dpooled = Flat(torch.zeros(B, C), fill=NAN).arm()
    grads = {k: Flat(v).arm() for k, v in p.old.items()}
    if params:
        bufs.update(grads)
    d = _se_desc(p, bufs)
    _ok(_lib().dyk_se_fc_bwd(ctypes.byref(d), None), "dyk_se_fc_bwd")
    for f in ins.values():
        f.assert_untouched()
    ws.assert_outside_untouched()
    w = ws.t.cpu()
    h, dt1, t2 = w[:B * Cs].view(B, Cs), w[B * Cs:2 * B * Cs].view(B, Cs), w[2 * B * Cs:].view(B, C)
    assert O.same_bits(h, p.h) == 0 and O.same_bits(t2, p.t2) == 0, "the backward call wrote into h or t2"
    if data:
        dpooled.assert_outside_untouched()
        _report("se_fc-dt1", "f32", *O.check(dt1, *O.se_dt1(p.h, p.t2, p.dscale, p.w2)), case)
        _report("se_fc-dpooled", "f32", *O.check(dpooled.t.cpu(), *O.se_dpooled(dt1, p.w1)), case)
    else:
        assert O.same_bits(dt1, p.dt1) == 0, "the parameter half wrote into dt1"
    for k, f in grads.items():
        if params:
            f.assert_outside_untouched()
        else:
            f.assert_untouched()
    if params:
        ref = O.se_wgrad(p.pooled, p.h, dt1, p.t2, p.dscale, p.old)
        for k, f in grads.items():
            _report("se_fc-" + k, "f32", *O.check(f.t.cpu(), *ref[k]), case)


def test_se_fc_backward_refuses_more_than_256_images():
    p = EC.se_problem(8, 4, 1)
    bufs = _se_inputs(p)
    bufs.update(dscale=Flat(p.dscale), ws=Flat(torch.zeros(257 * 16)), dpooled=Flat(torch.zeros(257, 8)))
    d = _se_desc(p, bufs)
    d.B = 257
    assert _lib().dyk_se_fc_bwd(ctypes.byref(d), None) == -1          # DYK_ERR_ARG


@pytest.mark.parametrize("H,W", EC.SE_SCALE_MAPS)
@pytest.mark.parametrize("dt,C", EC.SE_SCALE_C + [("f16", 8)])
def test_se_scale(dt, C, H, W):
    """out = a * p0[b, c] (+ p1[b, c] * alpha), store and accumulate"""
    B = 2
    a, old = EC.rand_tensor(B, C, H, W, dt, 51), EC.rand_tensor(B, C, H, W, dt, 52)
    g = torch.Generator().manual_seed(C + H)
    p0v, p1v = torch.rand(B, C, generator=g), torch.randn(B, C, generator=g)
    alpha = 1.0 / (H * W)
    for i, (has_p1, accumulate) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        lay = ("tight", "slice")[i % 2]
        case = "se_scale %dx%d c%d p1=%d acc=%d %s" % (H, W, C, has_p1, accumulate, lay)
        abuf = EC.nhwc(a, dt, lay)
        obuf = EC.nhwc(old, dt, _other(lay), fill=accumulate)
        p0, p1 = Flat(p0v).arm(), Flat(p1v).arm()
        d = _desc(dt, C, a=abuf, out=obuf, B=B, H=H, W=W, alpha=alpha, p0=p0, p1=p1 if has_p1 else None,
                  flags=_L().EW_ACCUM if accumulate else 0)
        _ok(_lib().dyk_se_scale(ctypes.byref(d), None), "dyk_se_scale")
        for f in (abuf, p0, p1):
            f.assert_untouched()
        obuf.assert_outside_untouched()
        tgt, bound = O.se_scale(a, p0v, EC.DTYPES[dt], p1v if has_p1 else None, alpha, old if accumulate else None)
        _report("se_scale", dt, *O.check(_nchw(obuf), tgt, bound), case)


def _se_scale_reduce(dt, B, C, H, W, act, slots, has_p1, accumulate, lay, case):
    """dyk_se_scale with `red`: the stored gradient has the bits of the plain launch; the replica sums, per channel, against fp64 sums
    formed from that stored gradient"""
    L = _L()
    dz, yraw, old, p0v, p1v, vecs = EC.se_reduce_problem(B, C, H, W, dt)
    alpha = 1.0 / (H * W)
    outs = []
    for reduce in (False, True):
        abuf, ybuf = EC.nhwc(dz, dt, lay), EC.nhwc(yraw, dt, _other(lay))
        obuf = EC.nhwc(old, dt, lay, fill=accumulate)
        p0, p1, p2 = Flat(p0v).arm(), Flat(p1v).arm(), Flat(vecs).arm()
        red = Flat(torch.zeros(slots, 2, C, dtype=torch.float64)).arm()
        d = _desc(dt, C, a=abuf, b=ybuf if reduce else None, out=obuf, B=B, H=H, W=W, alpha=alpha, p0=p0, p1=p1 if has_p1 else None,
                  p2=p2 if reduce else None, red=red if reduce else None, act=L.ACT_CODES[act], slots=slots,
                  flags=L.EW_ACCUM if accumulate else 0)
        _ok(_lib().dyk_se_scale(ctypes.byref(d), None), "dyk_se_scale")
        for f in (abuf, ybuf, p0, p1, p2):
            f.assert_untouched()
        obuf.assert_outside_untouched()
        red.assert_outside_untouched()
        outs.append(obuf.t.cpu())
    _exact("se_scale-with-reduce", dt, outs[1], outs[0], case)
    tgt, bound = O.se_scale(dz, p0v, EC.DTYPES[dt], p1v if has_p1 else None, alpha, old if accumulate else None)
    _report("se_scale", dt, *O.check(_nchw(obuf), tgt, bound), case)
    S, b = O.se_reduce(_nchw(obuf), yraw, vecs, act, EC.se_reduce_m(C, dt, B, H * W))
    got = red.t.cpu().sum(0)
    _report("se_scale-s1-" + act, dt, *O.check(got[0], S[0], b[0]), case)
    _report("se_scale-s2-" + act, dt, *O.check(got[1], S[1], b[1]), case)


@pytest.mark.parametrize("H,W", EC.SE_SCALE_MAPS)
@pytest.mark.parametrize("dt,C", EC.SE_SCALE_C)
def test_se_scale_with_the_batchnorm_backward_reduce(dt, C, H, W):
    """every activation the switch names (mish, relu, hard-swish, relu6) and the runtime default (leaky, linear); 1, 4 and 32 replicas"""
    for i, act in enumerate(O.REDUCE_ACTS):
        slots = (1, 4, 32)[i % 3]
        _se_scale_reduce(dt, 2, C, H, W, act, slots, i % 2 == 0, i % 4 >= 2, ("tight", "slice")[i % 2],
                         "se_scale+reduce %dx%d c%d %s slots%d" % (H, W, C, act, slots))


def test_se_scale_reduce_walks_several_images():
    """(32, 264, 25, 32): 26 workgroups per image plane, 29 along the images: three of them take a second image"""
    B, C, H, W = EC.SE_SCALE_LOOP
    assert EC.se_scale_geo(C, "bf16", B, H * W, True)[4] == 29 < B
    _se_scale_reduce("bf16", B, C, H, W, "hard-swish", 4, True, False, "tight", "se_scale+reduce 25x32 c264 b32")


# ---------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ny,nx", EC.HEAD_MAPS)
def test_head(ny, nx, B):
    """permute forward exact; backward the exact rounding into f32 / bf16 rows of ld channels with zero padding; the bias gradient on top of
    non-zero contents, and not touched when NULL"""
    L = _L()
    na, no = EC.HEAD_NA, EC.HEAD_NO
    g = torch.Generator().manual_seed(ny * nx + B)
    dp = torch.randn(B, na, ny, nx, no, generator=g)
    dpf = Flat(dp).arm()
    old = torch.randn(na * no, generator=g)
    for dt, lds in EC.HEAD_LD.items():
        for i, ld in enumerate(lds):
            case = "head %dx%d b%d ld%d" % (ny, nx, B, ld)
            if dt == "f32":
                y = torch.randn(B, ny, nx, ld, generator=g)
                yf = Flat(y).arm()
                pf = Flat(torch.zeros(B, na, ny, nx, no), fill=NAN).arm()
                _ok(_lib().dyk_head_permute_fwd(_ptr(yf), _ptr(pf), B, ny, nx, na, no, ld, None), "dyk_head_permute_fwd")
                yf.assert_untouched()
                pf.assert_outside_untouched()
                _exact("head-fwd", dt, pf.t.cpu(), O.head_fwd(y[..., :na * no].contiguous(), na, no), case)
            dy = Flat(torch.zeros(B, ny, nx, ld, dtype=EC.DTYPES[dt]), fill=EC.SENTINEL).arm()
            with_bias = i % 2 == 0
            db = Flat(old).arm()
            code = {"f32": L.DYK_F32, "bf16": L.DYK_BF16}[dt]
            _ok(_lib().dyk_head_permute_bwd(_ptr(dpf), _ptr(dy), _ptr(db) if with_bias else None, B, ny, nx, na, no, ld, code, None),
                "dyk_head_permute_bwd")
            dpf.assert_untouched()
            dy.assert_outside_untouched()
            _exact("head-bwd", dt, dy.t.cpu(), O.head_bwd(dp, ld, EC.DTYPES[dt]), case)
            if with_bias:
                db.assert_outside_untouched()
                _report("head-bias", "f32", *O.check(db.t.cpu(), *O.head_bias(dp, old)), case)
            else:
                db.assert_untouched()
