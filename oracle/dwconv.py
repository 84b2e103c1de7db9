"""fp64 restatement of the depthwise convolution (csrc/dwconv.hip: dyk_dwconv_fwd / dyk_dwconv_dgrad / dyk_dwconv_wgrad,
nn.Conv2d(groups=C) of reference models.py:41 and layers.py:223) and DERIVED per-element bounds on what an fp32 evaluation
of the same sums, stored in fp32, bf16 or fp16, may differ by.  Plain torch on the CPU, tap by tap; no bound is tuned
against the kernels.

Layout: x [B, C, Hi, Wi], dy [B, C, Ho, Wo], w tap-major [k*k, C] (the fp32 master copy the kernels read).  The caller
rounds x and dy to the storage type first; the reference then takes them as exact.

    y[b, c, yo, xo]  = sum_t x[b, c, yo*s + kh - pad, xo*s + kw - pad] * w[t, c]          t = kh*k + kw
    dx[b, c, yi, xi] = sum_t dy[b, c, (yi + pad - kh)/s, (xi + pad - kw)/s] * w[t, c]     where divisible and in range
    dw[t, c]         = sum_p dy[p, c] * x[src(p, t), c]
    S1[c] = sum y,  S2[c] = sum y^2                                                        (BatchNorm statistics)

and the same sums over absolute values: A_y = sum |x||w|, A_dx = sum |dy||w|, A_dw = sum |dy * x|.

Bounds.  u = 2^-24 is the unit roundoff of fp32, T = k*k the number of taps.

  forward / data gradient   T multiply-adds into an fp32 accumulator, fused or not, in any order, deviate from the exact sum
                            by at most T*u*A (products rounded: 2 roundings per tap, each on a partial sum <= A) to first
                            order; e = 2*T*u*A covers both forms and the second-order terms.
        fp32 storage        |got - ref| <= e
        16-bit storage      |got - ref| <= e + ulp_T(|ref| + e) / 2          (round to nearest of a value within e of ref)
                            ulp_T: the spacing of the bf16 grid (8 significant bits) or of the fp16 grid (11 bits, 2^-24 below
                            2^-14); fp16 stores SATURATE at +-65504 (tests/test_gpu_fp16.py), so ref is clamped there first
        A == 0              no tap reaches the element: bound 0, the output is exactly 0
  accumulate form           out = T(old + acc): the reference is ref + old, e' = e + u*|ref + old| (one more fp32 addition), then
                            the same rule with e'
  statistics                summed from the fp32 accumulators (error e each) in fp32 partial sums of at most n = B*Ho*Wo
                            terms, the partial sums then in fp64:
                            |s1 - S1| <= sum e + n*u*sum|y|
                            |s2 - S2| <= sum (2|y|e + e^2 + u*y^2) + n*u*sum y^2
  weight gradient           n products and n additions in fp32, any order, atomics or planes summed in fp64 on the host:
                            |dw - DW| <= (n + 1)*u*A_dw per (tap, channel)
"""
import torch

U = 2.0 ** -24
F16_MAX = 65504.0
_F64 = torch.float64


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def store(t, dtype):
    """the store rule of the kernels: round to nearest even; fp16 saturates first"""
    if dtype == torch.float16:
        return t.float().clamp(-F16_MAX, F16_MAX).half()
    return t.float().to(dtype)


def ulp(v, dtype):
    """spacing of the storage grid of `dtype` at magnitude |v| (float64 in, float64 out)"""
    v = v.abs().to(_F64)
    if dtype == torch.float16:
        bits, emin = 10, -14
        v = v.clamp(max=F16_MAX)
    elif dtype == torch.bfloat16:
        bits, emin = 7, -126
    else:
        bits, emin = 23, -126
    _, e = torch.frexp(v)                                  # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    e = torch.where(v > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
    return torch.exp2((e - bits).to(_F64))


def _padded(t, pad):
    return torch.nn.functional.pad(t, (pad, pad, pad, pad))


def _taps(k):
    return [(kh, kw, kh * k + kw) for kh in range(k) for kw in range(k)]


class Reference:
    """every fp64 quantity of one problem (attributes y, dx, dw, S1, S2, A_y, A_dx, A_dw, n, T; dx / dw / A_dx / A_dw only with dy)"""


def reference(x, w, dy, k, stride, pad):
    x, w = x.to(_F64), w.to(_F64)
    B, C, Hi, Wi = x.shape
    Ho, Wo = out_size(Hi, k, stride, pad), out_size(Wi, k, stride, pad)
    assert Ho >= 1 and Wo >= 1 and w.shape == (k * k, C)
    r = Reference()
    r.k, r.stride, r.pad, r.T, r.n = k, stride, pad, k * k, B * Ho * Wo
    xp = _padded(x, pad)
    ye, xe = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1          # extent of the strided window of one tap
    r.y = torch.zeros(B, C, Ho, Wo, dtype=_F64)
    r.A_y = torch.zeros_like(r.y)
    for kh, kw, t in _taps(k):
        win = xp[:, :, kh:kh + ye:stride, kw:kw + xe:stride]
        wt = w[t].view(1, C, 1, 1)
        r.y += win * wt
        r.A_y += win.abs() * wt.abs()
    r.S1, r.S2 = r.y.sum((0, 2, 3)), (r.y * r.y).sum((0, 2, 3))
    if dy is None:
        return r
    dy = dy.to(_F64)
    assert dy.shape == r.y.shape
    dxp = torch.zeros_like(xp)
    adxp = torch.zeros_like(xp)
    r.dw = torch.zeros(k * k, C, dtype=_F64)
    r.A_dw = torch.zeros_like(r.dw)
    for kh, kw, t in _taps(k):
        wt = w[t].view(1, C, 1, 1)
        dxp[:, :, kh:kh + ye:stride, kw:kw + xe:stride] += dy * wt
        adxp[:, :, kh:kh + ye:stride, kw:kw + xe:stride] += dy.abs() * wt.abs()
        prod = dy * xp[:, :, kh:kh + ye:stride, kw:kw + xe:stride]
        r.dw[t] = prod.sum((0, 2, 3))
        r.A_dw[t] = prod.abs().sum((0, 2, 3))
    crop = (slice(None), slice(None), slice(pad, pad + Hi), slice(pad, pad + Wi))
    r.dx, r.A_dx = dxp[crop].contiguous(), adxp[crop].contiguous()
    return r


def acc_error(A, T):
    """e: what the fp32 accumulator of T multiply-adds may be off by"""
    return 2.0 * T * U * A


def out_bound(ref, A, T, dtype, old=None):
    """(target, bound) of a stored forward / data-gradient element.  old: the accumulate form, out = dtype(old + acc)"""
    e = acc_error(A, T)
    tgt = ref
    if old is not None:
        tgt = ref + old.to(_F64)
        e = e + U * tgt.abs()
    if dtype == torch.float32:
        return tgt, e
    if dtype == torch.float16:
        tgt = tgt.clamp(-F16_MAX, F16_MAX)
    b = e + 0.5 * ulp(tgt.abs() + e, dtype)
    if old is None:
        b = torch.where(A == 0, torch.zeros_like(b), b)
    return tgt, b


def stats_bound(r):
    """bounds of the per-channel sums s1, s2 taken from the fp32 accumulators"""
    e = acc_error(r.A_y, r.T)
    y = r.y
    b1 = e.sum((0, 2, 3)) + r.n * U * y.abs().sum((0, 2, 3))
    b2 = (2 * y.abs() * e + e * e + U * y * y).sum((0, 2, 3)) + r.n * U * (y * y).sum((0, 2, 3))
    return b1, b2


def dw_bound(r):
    return (r.n + 1) * U * r.A_dw


def check(got, ref, bound):
    """(largest error / bound over the elements with a non-zero bound, number of elements outside their bound).  Elements whose
    bound is 0 must be equal; a non-finite value is outside any bound."""
    got, ref, bound = got.to(_F64), ref.to(_F64), bound.to(_F64)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    bad = int((err > bound).sum())
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return ratio, bad
