"""fp16 inference mode on the GPU (DYK_F16: IEEE half storage, v_mfma_f32_16x16x32_f16, fp32 accumulation, SATURATING stores).

Kernel level: conversions, every forward convolution configuration the tuner may hand a 16-bit problem, saturation (and why:
the tight-row over-read), the non-conv forward kernels.  Model level: per section on identical inputs, AP on the 64-pair fixture,
the MobileNetV3 cfg against bf16, the boundaries of the mode, stale weight copies.

Bounds.  u = 2^-11 is the unit roundoff of fp16, one ulp of a stored value v is at most 2^-10 |v|.  An fp32 sum of K products in
any order deviates from the exact one by at most K 2^-23 sum|x||w| (to first order).  So a stored fp16 result of a convolution
may deviate from the fp32 CPU result `ref` on the same fp16-rounded operands by
    2^-10 |ref|  +  K 2^-23 conv(|x|, |w|),       K = taps x Cin
(half an ulp of rounding, and a sum that landed on the other side of a tie); through a folded BatchNorm + activation the second
term is scaled by |scale| and the activation's Lipschitz constant (<= 1.09 for Mish) and nothing else is added: the few fp32 ulps
of the epilogue arithmetic sit inside it (K >= 24 here).  fp32 outputs (heads) lack the first term.
With a residual the kernels round the activation's value z to the storage type BEFORE the residual is added (as the bf16 path
does: the value a separate pass would read back).  That rounding is part of the REFERENCE, r16(mish(u)) + r, not of the bound.
One case remains: where z lies within the summation term of a rounding tie of fp16, the kernel's z and the reference's may round
to different neighbours, one fp16 ulp of z apart, and both are correct roundings of sums inside the bound.  Those elements, and
only those (`_tie_flip`: a fraction of about 2 * delta / ulp of them), get one ulp of z more."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import C1, C5, GOLDEN
from test_fp16_host import F16_EDGE_VALUES, f16_reference_bits

pytestmark = pytest.mark.gpu

F16 = torch.float16
F16_MAX = 65504.0
EPS32 = 2.0 ** -23


def r16(t):
    """the store rule of the fp16 path"""
    return t.clamp(-F16_MAX, F16_MAX).half().float()


def _tie_flip(z, delta):
    """one fp16 ulp of z where z is within delta of a rounding tie of the fp16 grid (ulp = 2^(e - 10), 2^-24 below 2^-14), else 0"""
    e = torch.floor(torch.log2(z.abs().clamp_min(2.0 ** -14)))
    u = torch.exp2(e - 10)
    frac = torch.remainder(z.abs().double() / u.double(), 1.0)
    return torch.where(((frac - 0.5).abs() * u.double()).float() <= delta, u, torch.zeros_like(u))


def _bits(t16):
    return t16.contiguous().view(torch.int16).to(torch.int64) & 0xffff


# ------------------------------------------------------------------------------------------------ 4. conversions
@pytest.mark.parametrize("C", [3, 8, 24])
def test_layout_conversions_round_like_clamp_then_half(C):
    from dyk import ops
    g = torch.Generator().manual_seed(4)
    vals = torch.cat([torch.tensor(F16_EDGE_VALUES, dtype=torch.float32), torch.randn(4096, generator=g)])
    per = C * 5 * 7
    B = -(-vals.numel() // per)
    x = torch.zeros(B * per)
    x[:vals.numel()] = vals
    x = x.view(B, C, 5, 7).contiguous()
    cpad = -(-C // 8) * 8
    xd = ops.to_nhwc(x.cuda(), F16, cpad=cpad)                     # ragged vectors (C = 3), padded rows
    assert xd.dtype == F16 and xd.shape == (B, 5, 7, cpad)
    ref = r16(x)
    got16 = xd[..., :C].permute(0, 3, 1, 2).cpu()
    nan = torch.isnan(x)
    assert torch.equal(_bits(got16)[~nan], f16_reference_bits(x)[~nan])
    assert bool(torch.isnan(got16[nan]).all()) and not bool(torch.isinf(got16.float()).any())
    if cpad > C:
        assert float(xd[..., C:].float().abs().max()) == 0.0        # padding channels are zero
    back = ops.to_nchw(xd, C=C).cpu()
    assert torch.equal(back[~nan].view(torch.int32), ref[~nan].view(torch.int32)) and bool(torch.isnan(back[nan]).all())


def test_cast_f32_rounds_like_clamp_then_half():
    from dyk import lib as L
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.tensor(F16_EDGE_VALUES, dtype=torch.float32), torch.randn(4096, generator=g),
                   torch.randn(1023, generator=g) * 3e4])          # (n % 4 != 0: the scalar tail)
    src = x.cuda()
    dst = torch.zeros(x.numel() + 8, dtype=F16, device="cuda")
    L.check(L.load().dyk_cast_f32(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), x.numel(), L.DYK_F16,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dyk_cast_f32")
    got = dst[:x.numel()].cpu()
    nan = torch.isnan(x)
    assert torch.equal(_bits(got)[~nan], f16_reference_bits(x)[~nan])
    assert bool(torch.isnan(got[nan]).all()) and float(dst[x.numel():].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. convolutions
def _tight(t, C, dtype=F16, spare=256):
    """channels-last rows of exactly C (multiple of 8) elements + spare zero elements behind the tensor (the arena's K-tail pad)"""
    from dyk import ops
    n = t.shape[0] * t.shape[2] * t.shape[3]
    flat = torch.zeros(n * C + spare, dtype=dtype, device="cuda")
    v = flat[:n * C].view(t.shape[0], t.shape[2], t.shape[3], C)
    ops.to_nhwc(t.cuda(), dtype, out=v)
    return flat, v


def _family(tune, S):
    tile = (tune >> 12) & 0xf
    fam = {5: "large-tile", 7: "pointwise", 3: "halo", 4: "halo"}.get(tile, "generic")
    if (tune >> 28) & 7 == 1:
        fam = "k-grouped"
    return fam + ("+split-K" if S > 1 else "")


class _ConvProblem:
    """one convolution problem: operands on the GPU (tight rows, K padded in the weight pack only), CPU fp32 references and
    per-element bounds of the four epilogue forms -- computed once, shared by every candidate"""

    def __init__(self, B, H, W, Cin, Cout, k, stride, seed, xscale=1.0, wscale=None, denormal=False):
        from dyk import ops
        g = torch.Generator().manual_seed(seed)
        self.k, self.stride, self.pad, self.Cin, self.Cout = k, stride, k // 2, Cin, Cout
        K = k * k * Cin
        if denormal:
            x = (torch.rand(B, Cin, H, W, generator=g) + 1.0) * 2.0 ** -16 * (torch.randint(0, 2, (B, Cin, H, W), generator=g) * 2.0 - 1.0)
            w = torch.randn(Cout, Cin, k, k, generator=g)
        else:
            x = torch.randn(B, Cin, H, W, generator=g) * xscale
            w = torch.randn(Cout, Cin, k, k, generator=g) * (wscale if wscale is not None else K ** -0.5)
        x, w = r16(x), r16(w)
        self.x, self.w = x, w
        pad = self.pad
        y = F.conv2d(x, w, stride=stride, padding=pad)
        sab = F.conv2d(x.abs(), w.abs(), stride=stride, padding=pad)        # conv(|x|, |w|)
        self.Ho, self.Wo = y.shape[2], y.shape[3]
        r = r16(torch.randn(y.shape, generator=g))
        scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
        bias = torch.randn(Cout, generator=g) * (0.0 if denormal else 1.0)      # (denormal case: the tiny sums alone, unrounded)
        sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
        sumt = K * EPS32 * sab
        u = y * sc + sh
        zm = F.mish(u)
        zl = F.leaky_relu(u, 0.1)
        self.forms = {
            # name: (kwargs of conv2d_fwd, reference, bound)
            "plain": (dict(), y, 2.0 ** -10 * y.abs() + sumt),
            "affine+mish+res": (dict(act="mish", scale=scale.cuda(), shift=shift.cuda(), res="r"), r16(zm) + r,
                                2.0 ** -10 * (r16(zm) + r).abs() + 1.09 * sc * sumt + _tie_flip(zm, 1.09 * sc * sumt)),
            "affine+leaky": (dict(act="leaky", scale=scale.cuda(), shift=shift.cuda()), zl, 2.0 ** -10 * zl.abs() + sc * sumt),
            "out_f32": (dict(shift=bias.cuda(), out_f32=True), y + bias.view(1, -1, 1, 1), sumt),
        }
        self.Kp = -(-Cin // 32) * 32
        self.xflat, self.xd = _tight(x, Cin)
        self.rflat, self.rd = _tight(r, Cout)
        self.wp = ops.pack_weight(w.cuda(), F16, cin_pad=self.Kp)
        self.dev = {n: (ref.cuda(), bnd.cuda()) for n, (_, ref, bnd) in self.forms.items()}

    def launch(self, form, tune, S=0):
        """-> NCHW fp32 result on the GPU, or None when the library answers DYK_ERR_UNSUPPORTED"""
        from dyk import lib as L, ops
        kw = dict(self.forms[form][0])
        of32 = kw.pop("out_f32", False)
        res = self.rd if kw.pop("res", None) else None
        B = self.x.shape[0]
        n = B * self.Ho * self.Wo
        flat = torch.full((n * self.Cout + 64,), float("nan"), dtype=torch.float32 if of32 else F16, device="cuda")
        out = flat[:n * self.Cout].view(B, self.Ho, self.Wo, self.Cout)
        d = ops.make_conv_desc(self.xd, self.wp, out, Hi=self.x.shape[2], Wi=self.x.shape[3], Cin=self.Kp, Cout=self.Cout,
                               Hg=self.Ho, Wg=self.Wo, Ho=self.Ho, Wo=self.Wo, taps=ops.fwd_taps(self.k, self.pad),
                               isy=self.stride, isx=self.stride, res=res, out_f32=of32, ldx=self.Cin, **kw)
        d.tune = tune
        keep = ops.attach_splitk(d, S, "cuda") if S > 1 else None
        if S > 1 and keep is None:
            return None
        rc = L.load().dyk_conv_igemm(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc == -3:                                                     # DYK_ERR_UNSUPPORTED
            return None
        assert rc == 0, (form, hex(tune), S, rc)
        self.last_flat = flat
        return ops.to_nchw(out) if not of32 else out.permute(0, 3, 1, 2)

    def candidates(self):
        from dyk import ops
        from dyk.plan import _conv_candidates, _conv_split_candidates
        out = torch.empty((self.x.shape[0], self.Ho, self.Wo, self.Cout), dtype=F16, device="cuda")
        probe = ops.make_conv_desc(self.xd, self.wp, out, Hi=self.x.shape[2], Wi=self.x.shape[3], Cin=self.Kp, Cout=self.Cout,
                                   Hg=self.Ho, Wg=self.Wo, Ho=self.Ho, Wo=self.Wo, taps=ops.fwd_taps(self.k, self.pad),
                                   isy=self.stride, isx=self.stride, ldx=self.Cin)
        return [(0, 0)] + [(t, 0) for t in _conv_candidates(probe)] + list(_conv_split_candidates(probe))

    def check(self, form, got, what):
        ref, bnd = self.dev[form]
        exc = ((got - ref).abs() - bnd).max().item()
        assert bool(torch.isfinite(got).all()) and exc <= 0.0, (what, form, "exceeds the bound by %.3g" % exc)


# (B, H, W, Cin, Cout, k, stride): ragged + tight rows with an over-read tail | large-tile, halo, K-grouped | split-K | pointwise
CONV_CASES = [(1, 9, 11, 24, 40, 1, 1), (1, 9, 11, 24, 40, 1, 2), (1, 9, 11, 24, 40, 3, 1), (1, 9, 11, 24, 40, 3, 2),
              (2, 16, 20, 128, 128, 3, 1), (1, 8, 20, 512, 96, 1, 1), (1, 8, 20, 128, 96, 1, 1)]
# families that must have run at least once on a case (the others may answer DYK_ERR_UNSUPPORTED for its shape)
CONV_MUST = {4: ("generic", "halo", "large-tile", "k-grouped"), 5: ("generic", "generic+split-K", "k-grouped"), 6: ("generic", "pointwise")}


@pytest.mark.parametrize("ci", range(len(CONV_CASES)), ids=lambda i: "b%d_%dx%d_c%d_%d_k%d_s%d" % CONV_CASES[i])
def test_every_forward_conv_configuration_in_fp16(ci):
    B, H, W, Cin, Cout, k, stride = CONV_CASES[ci]
    pr = _ConvProblem(B, H, W, Cin, Cout, k, stride, seed=50 + ci)
    ran = {}
    for tune, S in pr.candidates():
        tile = (tune >> 12) & 0xf
        # large-tile / pointwise / halo / K-grouped: no silent fallback to the generic tile (the family counts below are real)
        nofb = (1 << 23) if tile in (3, 4, 5, 7) or (tune >> 28) & 7 == 1 else 0
        for form in pr.forms:
            if tile == 7 and form != "plain":
                continue                                                # (the pointwise kernels store raw sums only)
            if tile == 5 and form == "out_f32":
                continue
            got = pr.launch(form, tune | nofb, S)
            if got is None:
                continue
            pr.check(form, got, (hex(tune), S))
            ran[_family(tune, S)] = ran.get(_family(tune, S), 0) + 1
    print("case %s: launches per family %s" % (CONV_CASES[ci], ran))
    assert ran.get("generic", 0) >= 4
    for fam in CONV_MUST.get(ci, ()):
        assert ran.get(fam, 0) >= 1, (fam, ran)


def test_fp16_denormal_operands_contribute():
    """x in the fp16 DENORMAL range (2^-16 .. 2^-15), w ~ 1: the matrix cores must not flush them.  fp32 output, so that the
    result itself is not subject to fp16 rounding: the bound is the summation term alone."""
    pr = _ConvProblem(1, 9, 11, 24, 40, 3, 1, seed=77, denormal=True)
    assert float(pr.x.abs().max()) < 2.0 ** -14 and float(pr.x.abs().min()) >= 2.0 ** -16
    ref, _ = pr.dev["out_f32"]
    got = pr.launch("out_f32", 0)
    pr.check("out_f32", got, "denormal operands")
    # not vanished: the operands' own contribution dominates the bias-free part of the output
    bias = pr.forms["out_f32"][0]["shift"].view(1, -1, 1, 1)
    part = (got - bias).abs().max().item()
    assert part > 0.5 * (ref - bias).abs().max().item() > 0.0


# ------------------------------------------------------------------------------------------------ 6. saturation
@pytest.mark.parametrize("k", [1, 3])
def test_stores_saturate_and_the_tight_row_overread_stays_finite(k):
    from dyk import ops
    pr = _ConvProblem(1, 6, 7, 24, 16, k, 1, seed=60 + k, xscale=1.0, wscale=1.0)
    g = torch.Generator().manual_seed(61)
    x = r16((torch.rand(pr.x.shape, generator=g) * 2 - 1) * 6e4)
    pr.x = x
    pr.xflat, pr.xd = _tight(x, 24)
    K = k * k * 24
    y = F.conv2d(x, pr.w, padding=k // 2)
    sumt = K * EPS32 * F.conv2d(x.abs(), pr.w.abs(), padding=k // 2)
    assert float((y.abs() > F16_MAX).float().mean()) > 0.3
    pr.dev["plain"] = (y.cuda(), (2.0 ** -10 * y.abs() + sumt).cuda())
    got = pr.launch("plain", 0).cpu()
    raw = pr.last_flat                                                   # the whole buffer, padded tail included
    n = 6 * 7 * 16
    assert bool(torch.isfinite(raw[:n].float()).all()), "inf / NaN in the output"
    assert bool(torch.isnan(raw[n:]).all()), "the launch wrote behind its tensor"
    over, under = y > F16_MAX + sumt, y < -F16_MAX - sumt
    inside = y.abs() < F16_MAX - sumt - 32.0
    assert bool((got[over] == F16_MAX).all()) and bool((got[under] == -F16_MAX).all())
    assert float(got.abs().max()) == F16_MAX
    assert bool(((got - y).abs() <= 2.0 ** -10 * y.abs() + sumt)[inside].all())
    # the saturated tensor as the input of a 16 -> 24 1x1 conv with TIGHT rows: its last K step over-reads the next pixel's
    # first channels (+-65504 here) against zero weight rows -- finite x 0; an inf there would be NaN in every output
    w2 = r16(torch.randn(24, 16, 1, 1, generator=g) / 64)
    sat = torch.zeros(n + 256, dtype=F16, device="cuda")
    sat[:n] = raw[:n]
    xd2 = sat[:n].view(1, 6, 7, 16)
    wp2 = ops.pack_weight(w2.cuda(), F16, cin_pad=32)
    out = torch.full((1, 6, 7, 24), float("nan"), dtype=F16, device="cuda")
    d = ops.make_conv_desc(xd2, wp2, out, Hi=6, Wi=7, Cin=32, Cout=24, Hg=6, Wg=7, Ho=6, Wo=7, taps=ops.fwd_taps(1, 0), ldx=16)
    from dyk import lib as L
    L.check(L.load().dyk_conv_igemm(ctypes.byref(d), None), "dyk_conv_igemm")
    got2 = ops.to_nchw(out).cpu()
    y2 = F.conv2d(got, w2)
    b2 = 2.0 ** -10 * y2.abs() + 16 * EPS32 * F.conv2d(got.abs(), w2.abs())
    assert bool(torch.isfinite(got2).all())
    assert bool(((got2 - r16(y2)).abs() <= b2).all()), float(((got2 - r16(y2)).abs() - b2).max())


# ------------------------------------------------------------------------------------------------ 7. other forward kernels
def _ulp16(t):
    """one fp16 ulp of |t|: at most 2^-10 |t| for a normal result, the fixed step 2^-24 of the denormal grid below 2^-14
    (denormals are kept, so a result there is rounded to that grid: a relative bound alone would ask for more than the format has)"""
    return (2.0 ** -10 * t.abs()).clamp_min(2.0 ** -24)


def _within(got, ref, bound, what):
    exc = float(((got - ref).abs() - bound).max())
    assert bool(torch.isfinite(got).all()) and exc <= 0.0, (what, "exceeds the bound by %.3g" % exc)


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("W", [10, 12])          # 12: the uint8 MFMA kernel (W % 4 == 0); 10: the scalar kernel
def test_stem_forward_in_fp16(u8, stride, W):
    from dyk import lib as L
    B, H, cout = 2, 6, 32
    g = torch.Generator().manual_seed(70 + stride + W)
    img8 = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g)
    imgf = img8.float() / 255.0
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.3
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    y = F.conv2d(imgf, w, stride=stride, padding=1)
    sab = F.conv2d(imgf, w.abs(), stride=stride, padding=1)
    sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    img = (img8 if u8 else imgf).cuda().contiguous()
    wt = w.permute(0, 2, 3, 1).contiguous().view(cout, 27).t().contiguous().cuda()
    d = L.DykStemDesc()
    d.img, d.in_u8, d.dtype = img.data_ptr(), 1 if u8 else 0, L.DYK_F16
    d.B, d.H, d.W, d.Cout, d.k, d.stride, d.pad = B, H, W, cout, 3, stride, 1
    d.Ho, d.Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for affine in (False, True):
        out = torch.full((B, d.Ho, d.Wo, cout), float("nan"), dtype=F16, device="cuda")
        d.wt, d.y, d.ldy = wt.data_ptr(), out.data_ptr(), cout
        sd_, sh_ = scale.cuda(), shift.cuda()
        d.scale, d.shift, d.act = (sd_.data_ptr(), sh_.data_ptr(), L.ACT_CODES["leaky"]) if affine else (None, None, 0)
        L.check(L.load().dyk_stem_conv_fwd(ctypes.byref(d), stream), "dyk_stem_conv_fwd")
        got = out.float().cpu().permute(0, 3, 1, 2)
        ref = F.leaky_relu(y * sc + sh, 0.1) if affine else y
        # 27 products (+ the uint8 kernel's 1/255 behind the sum, the three-term weight split: a few fp32 ulps of the terms)
        bound = _ulp16(ref) + (27 + 8) * EPS32 * sab * (sc if affine else 1.0) + (16 * EPS32 * (y.abs() * sc + sh.abs()) if affine else 0.0)
        _within(got, ref, bound, ("stem", u8, stride, W, affine))
    # the inference type has no statistics epilogue and no weight gradient
    st = torch.zeros(4, 2 * cout, dtype=torch.float64, device="cuda")
    d.stats, d.stats_slots = st.data_ptr(), 4
    assert L.load().dyk_stem_conv_fwd(ctypes.byref(d), stream) == -3


@pytest.mark.parametrize("C", [8, 24])
def test_elementwise_forward_kernels_in_fp16(C):
    from dyk import lib as L, ops
    B, H, W = 2, 6, 10
    g = torch.Generator().manual_seed(80 + C)
    x = r16(torch.randn(B, C, H, W, generator=g) * 3)
    x2 = r16(torch.randn(B, C, H, W, generator=g))
    xd, x2d = ops.to_nhwc(x.cuda(), F16), ops.to_nhwc(x2.cuda(), F16)
    ulp = _ulp16
    # depthwise 3x3, stride 1 (LDS-tiled / strip kernel) and 2 (generic kernel); fp32 weights
    wdw = torch.randn(C, 1, 3, 3, generator=g) * 0.4
    wt = wdw.view(C, 9).t().contiguous().cuda()
    for stride in (1, 2):
        ref = F.conv2d(x, wdw, stride=stride, padding=1, groups=C)
        sab = F.conv2d(x.abs(), wdw.abs(), stride=stride, padding=1, groups=C)
        got = ops.to_nchw(ops.dwconv_fwd(xd, wt, 3, stride, 1)).cpu()
        _within(got, ref, ulp(ref) + 9 * EPS32 * sab, ("dwconv", stride))
    # squeeze-excitation: pool (fp32 out) and scale
    pooled = torch.zeros(B, C, device="cuda")
    ops.call("dyk_se_pool", ops.ew_desc(a=xd, B=B, H=H, W=W, alpha=1.0 / (H * W)), pooled)
    _within(pooled.cpu(), x.mean((2, 3)), (H * W + 2) * EPS32 * x.abs().mean((2, 3)), "se_pool")
    s = torch.rand(B, C, generator=g)
    s_d = s.cuda()
    z = torch.empty_like(xd)
    ops.call("dyk_se_scale", ops.ew_desc(a=xd, out=z, p0=s_d, B=B, H=H, W=W))
    ref = x * s.view(B, C, 1, 1)
    _within(ops.to_nchw(z).cpu(), ref, ulp(ref) + 2 * EPS32 * ref.abs(), "se_scale")
    # max pool 3 / 5 / 9 (ties through quantised values) and nearest upsampling: bit-exact
    xq = (x * 2).round() / 2
    xqd = ops.to_nhwc(xq.cuda(), F16)
    for k in (3, 5, 9):
        mp = torch.empty_like(xqd)
        amax = torch.zeros(B * H * W * C, dtype=torch.uint8, device="cuda")
        ops.call("dyk_maxpool_fwd", ops.ew_desc(a=xqd, out=mp, B=B, H=H, W=W, k=k), amax)
        assert torch.equal(ops.to_nchw(mp).cpu(), F.max_pool2d(xq, k, 1, (k - 1) // 2)), "maxpool k=%d" % k
    up = torch.empty(B, 2 * H, 2 * W, C, dtype=F16, device="cuda")
    ops.call("dyk_upsample2x_fwd", ops.ew_desc(a=xd, out=up, B=B, H=H, W=W))
    assert torch.equal(ops.to_nchw(up).cpu(), F.interpolate(x, scale_factor=2, mode="nearest"))
    # axpby: copy into a channel slice of a concat buffer, accumulate, weighted fusion
    cat = torch.zeros(B, H, W, C + 16, dtype=F16, device="cuda")
    ops.call("dyk_axpby", ops.ew_desc(a=xd, out=cat[..., 8:8 + C]))
    assert torch.equal(cat[..., 8:8 + C], xd) and float(cat[..., :8].float().abs().max()) == 0.0
    ops.call("dyk_axpby", ops.ew_desc(a=x2d, out=cat[..., 8:8 + C], flags=L.EW_ACCUM))
    ref = x + x2
    _within(ops.to_nchw(cat[..., 8:8 + C]).cpu(), ref, ulp(ref), "axpby accumulate")
    weff = torch.tensor([0.7, 1.3]).cuda()
    z = torch.empty_like(xd)
    ops.call("dyk_axpby", ops.ew_desc(a=xd, b=x2d, out=z, p0=weff[0:1], p1=weff[1:2]))
    ref = 0.7 * x + 1.3 * x2
    _within(ops.to_nchw(z).cpu(), ref, ulp(ref) + 4 * EPS32 * (0.7 * x.abs() + 1.3 * x2.abs()), "wfuse")
    # folded BatchNorm + activation
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    scale_d, shift_d = scale.cuda(), shift.cuda()
    for act, fn, lip in (("leaky", lambda t: F.leaky_relu(t, 0.1), 1.0), ("mish", F.mish, 1.09), ("relu6", F.relu6, 1.0)):
        z = torch.empty_like(xd)
        ops.call("dyk_bn_act_fwd", ops.ew_desc(a=xd, out=z, act=act, p0=scale_d, p1=shift_d))
        pre = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        ref = fn(pre)
        _within(ops.to_nchw(z).cpu(), ref, ulp(ref) + 16 * EPS32 * lip * ((x * scale.view(1, -1, 1, 1)).abs() + shift.abs().view(1, -1, 1, 1) + ref.abs()),
                ("bn_act", act))
    # training forms answer DYK_ERR_UNSUPPORTED
    red = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert L.load().dyk_dot(ctypes.byref(ops.ew_desc(a=xd, b=x2d, red=red[0:1])), None) == -3
    assert L.load().dyk_upsample2x_bwd(ctypes.byref(ops.ew_desc(a=up, out=z, C=C, B=B, H=H, W=W)), None) == -3


# ------------------------------------------------------------------------------------------------ model level
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))


def _fp16_state(net, sd):
    """the per-section reference: weights of plain, non-stem convolutions rounded as the fp16 weight copy is"""
    out = dict(sd)
    for i, Lr in enumerate(net.layers):
        if Lr["kind"] != "convolutional" or Lr["groups"] != 1:
            continue
        if i == 0 or (net.second_index is not None and i == net.second_index):
            continue
        k = "module_list.%d.Conv2d.weight" % i
        out[k] = r16(sd[k])
    return out


def _model(cfg, sd, dtype):
    from build_utils.parse_config import materialize_cfg
    from models import YOLO
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(cfg))
    m.load_state_dict(sd)
    m.dyk_dtype = dtype
    return m.cuda()


def test_fp16_path_section_by_section_on_identical_inputs(monkeypatch, tiles):
    """the 8-pair fixture of test_bf16_path_layer_by_layer...: every section of the fp16 plan against the oracle fed the HIP
    path's own tensors, within 2 fp16 ulps (2 * 2^-11) of the tensor's scale; heads (fp32 sums over identical operands) within
    2e-4; nothing saturates (the fixture's largest activation is 18.7); two runs are bit-identical."""
    import test_eval_ap as E
    monkeypatch.setenv("DYK_DEBUG_PLAN", "1")
    from gpu_debug_model import tref_to_nchw
    net, sd = E._state()
    v8, l8 = E.R2.eval_images()
    x, y = v8.float() / 255.0, l8.float() / 255.0
    m = _model(E.R2.EVAL_CFG, sd, "fp16").eval()
    with torch.no_grad():
        io, p = m(x.cuda(), y.cuda())
        io1, p1 = io.clone(), [q.clone() for q in p]
    torch.cuda.synchronize()
    plan = list(m.engine.plans.values())[0]
    assert plan.dtype is F16
    act1 = plan.arenas["act"].tensor.clone()
    hip = {}
    for i, t in enumerate(plan.outs):
        if t is not None and plan.info[i]["kind"] != "yolo" and t.esize == 2:
            hip[i] = tref_to_nchw(plan, t)
    with torch.no_grad():
        (io_e, p_e), every = net.forward(_fp16_state(net, sd), x, y, training=False, keep_all=True, force=hip)
    worst, checked = (0.0, -1), 0
    for i, got in hip.items():
        ref = r16(every[i])
        if got.shape != ref.shape:
            continue
        assert float(got.abs().max()) < F16_MAX, "section %d saturated" % i
        rel = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)
        worst = max(worst, (rel, i))
        checked += 1
        assert rel <= 2 * 2.0 ** -11, "section %d (%s): %.3g of the tensor's scale" % (i, plan.info[i]["kind"], rel)
    print("fp16 per-section (identical inputs): %d sections, worst deviation %.2e of scale at section %d" % (checked, worst[0], worst[1]))
    assert checked >= 250
    for a_, b_ in zip(p, p_e):
        assert float((a_.cpu() - b_).abs().max()) <= 2e-4 * float(b_.abs().max())
    with torch.no_grad():
        io2, p2 = m(x.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert torch.equal(io2, io1) and all(torch.equal(a_, b_) for a_, b_ in zip(p2, p1))
    assert torch.equal(plan.arenas["act"].tensor, act1)


def test_fp16_eval_ap_on_the_64_pair_fixture(monkeypatch, tiles):
    """AP / LAMR / detections of the fp16 path on tests/golden/evalap_trained64.npz (pinned tiles) against the fp32 reference and
    the oracle run in fp16-emulating arithmetic (the oracle's bf16 rounding hook swapped for clamp -> half inside this test)."""
    import test_eval_ap as E
    from build_utils.utils import non_max_suppression, scale_coords
    from oracle import metrics as ometrics, nms as onms
    from other_utils.metrics import compute_ap_lamr
    R5, GOLD5 = E.R5, E.GOLD5
    net, sd = E._state5()
    v, l, targets = R5.dataset()
    m = _model(R5.CFG, sd, "fp16").eval()
    with torch.no_grad():
        io = torch.cat([m(v[c:c + 16].cuda().float() / 255.0, l[c:c + 16].cuda().float() / 255.0)[0].clone() for c in range(0, 64, 16)])
    assert bool(torch.isfinite(io).all())
    dets = non_max_suppression(io, conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
    res, ndet = E._ap5(dets, scale_coords, compute_ap_lamr, targets)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "bfloat16", lambda t: t.clamp(-F16_MAX, F16_MAX).half())
        with torch.no_grad():
            io_e = torch.cat([net.forward(sd, v[c:c + 16].float() / 255.0, l[c:c + 16].float() / 255.0, training=False,
                                          emulate_bf16=True)[0] for c in range(0, 64, 16)])
    dets_e = onms.non_max_suppression(io_e, conf_thres=R5.CONF, iou_thres=R5.IOU, multi_label=False)
    emu, nde = E._ap5(dets_e, onms.scale_coords, ometrics.compute_ap_lamr, targets)
    gio = torch.from_numpy(GOLD5["io"])
    rel = float((io.cpu() - gio).abs().max()) / float(gio.abs().max())
    rel_e = float((io_e - gio).abs().max()) / float(gio.abs().max())
    ref_ap, ref_n = float(GOLD5["ap"]), int(GOLD5["ndet"].sum())
    print("64-pair fixture, fp16: AP %.5f LAMR %.5f %d detections, io rel. error %.3e | fp16-emulating oracle: AP %.5f LAMR %.5f %d "
          "detections, io rel. error %.3e | fp32 reference: AP %.5f LAMR %.5f %d detections"
          % (res["ap"], res["lamr"], ndet, rel, emu["ap"], emu["lamr"], nde, rel_e, ref_ap, float(GOLD5["lamr"]), ref_n))
    assert emu["ap"] - 3e-3 <= res["ap"] <= ref_ap + 1e-3, (res["ap"], emu["ap"], ref_ap)
    assert abs(res["ap"] - ref_ap) <= 1e-2, (res["ap"], ref_ap)
    assert rel <= 3 * rel_e, (rel, rel_e)
    assert abs(res["lamr"] - emu["lamr"]) <= 3e-2, (res["lamr"], emu["lamr"])
    assert abs(ndet - 910) <= 5, ndet


def test_fp16_on_the_mobilenetv3_cfg_against_bf16(tiles):
    """kaist_dyolov4_mobilenetv3_fshare_global_cse3 (depthwise, SE, hard-swish): head tensors of the fp16 and of the bf16 run
    against the fp32 oracle, error = max |delta| / max |ref| over the three heads; fp16 <= 0.25 x bf16 (2^-3 = the ratio of the
    rounding steps, x 2 for the max-norm)."""
    import make_golden_round4 as R4
    from helpers import oracle_net
    net = oracle_net(C5)
    sd = R4.conditioned_state(net.synth_state(5))
    g = torch.Generator().manual_seed(10)
    x8 = torch.randint(0, 256, (2, 3, 64, 96), dtype=torch.uint8, generator=g)
    y8 = torch.randint(0, 256, (2, 3, 64, 96), dtype=torch.uint8, generator=g)
    with torch.no_grad():
        _, p_ref = net.forward(sd, x8.float() / 255.0, y8.float() / 255.0, training=False)
    m = _model(C5, sd, "fp16").eval()
    err = {}
    for dt in ("fp16", "bf16"):
        m.dyk_dtype = dt
        with torch.no_grad():
            _, p = m(x8.cuda(), y8.cuda())
        assert all(bool(torch.isfinite(q).all()) for q in p)
        err[dt] = max(float((a_.cpu() - b_).abs().max()) for a_, b_ in zip(p, p_ref)) / max(float(b_.abs().max()) for b_ in p_ref)
    print("MobileNetV3 cfg, head error against the fp32 oracle: fp16 %.3e, bf16 %.3e, ratio %.3f" % (err["fp16"], err["bf16"], err["fp16"] / err["bf16"]))
    assert err["fp16"] <= 0.25 * err["bf16"], err


def _small(cfg=C1, seed=0):
    from helpers import oracle_net
    net = oracle_net(cfg)
    sd = net.synth_state(seed)
    g = torch.Generator().manual_seed(12)
    return sd, torch.rand(2, 3, 64, 96, generator=g).cuda(), torch.rand(2, 3, 64, 96, generator=g).cuda()


def test_fp16_boundaries(tiles, monkeypatch):
    monkeypatch.delenv("DYK_DTYPE", raising=False)
    sd, x, y = _small()
    # training in fp16 is refused at the first forward
    m = _model(C1, sd, "fp16").train()
    with pytest.raises(NotImplementedError, match="inference"):
        m(x, y)
    # an fp16 autocast region without dyk_dtype still means bf16
    m = _model(C1, sd, None).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m(x, y)
    assert [k[3] for k in m.engine.plans] == [torch.bfloat16]
    # plans and weight copies of the three types do not disturb one another
    m = _model(C1, sd, "fp32").eval()
    outs = {}
    with torch.no_grad():
        for dt in ("fp32", "bf16"):
            m.dyk_dtype = dt
            outs[dt] = m(x, y)[0].clone()
        m.dyk_dtype = "fp16"
        o16 = m(x, y)[0].clone()
        # (uncalibrated synth_state weights: activations saturate and the fp32 decode's exp() of the clipped heads may reach inf --
        # fp32 arithmetic, not a store of this path; what the saturating stores rule out is NaN from inf x 0)
        assert not bool(torch.isnan(o16).any()) and not torch.equal(o16, outs["bf16"]) and not torch.equal(o16, outs["fp32"])
        for dt in ("fp32", "bf16"):
            m.dyk_dtype = dt
            assert torch.equal(m(x, y)[0], outs[dt]), dt
        m.dyk_dtype = "fp16"
        assert torch.equal(m(x, y)[0], o16)
    assert sorted(str(k[3]) for k in m.engine.plans) == ["torch.bfloat16", "torch.float16", "torch.float32"]


@pytest.mark.parametrize("how", ["fused_adam", "torch_adam", "load_state_dict"])
def test_fp16_weight_copy_is_rebuilt_after_the_weights_change(how, tiles, monkeypatch):
    """fp16 eval forward -> the weights change (one bf16 train step with FusedAdam / torch.optim.Adam, or load_state_dict) ->
    fp16 eval forward: bit-equal to a fresh model loaded from the changed model's state_dict()"""
    monkeypatch.delenv("DYK_DTYPE", raising=False)
    sd, x, y = _small()
    m = _model(C1, sd, "fp16").eval()
    with torch.no_grad():
        before = m(x, y)[0].clone()
    if how == "load_state_dict":
        from helpers import oracle_net
        m.load_state_dict(oracle_net(C1).synth_state(1))
    else:
        m.dyk_dtype = "bf16"
        m.train()
        if how == "fused_adam":
            from dyk.optim import FusedAdam
            opt = FusedAdam(m, lr=1e-2)
        else:
            opt = torch.optim.Adam(m.parameters(), lr=1e-2)
        pred = m(x, y)
        loss = sum((q.float() ** 2).mean() for q in pred)
        loss.backward()
        opt.step()
        m.dyk_dtype = "fp16"
        m.eval()
    with torch.no_grad():
        after = m(x, y)[0].clone()
    assert not torch.equal(after, before)
    fresh = _model(C1, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, "fp16").eval()
    with torch.no_grad():
        want = fresh(x, y)[0]
    assert torch.equal(after, want)
