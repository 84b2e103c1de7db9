"""fp64 restatement of the channels-last kernels of csrc/elementwise.hip (axpby / dot, nearest 2x upsample, max pool with arg-max, the
squeeze-excitation chain, the YOLO head permute and its bias gradient; reference build_utils/layers.py:66-83, 185-189 and
models.py:91-94, 229) and DERIVED per-element bounds on what an fp32 evaluation, stored in fp32, bf16 or fp16, may differ by.  Plain torch
on the CPU, written from each operation's contract; no bound is tuned against a kernel and none depends on the association of a sum.

Notation: u = 2^-24, gamma(n) = n u / (1 - n u) (n roundings on one path, any association), ulp_T the spacing of the storage type.
`stored(tgt, e, T)` is the storage rule of oracle/stem.py: fp32 |got - tgt| <= e; bf16 / fp16 e + ulp_T(|tgt| + e) / 2 (fp16 clamps at
+-65504 first).  Tensors are NCHW here; the tests move them to and from the kernels' channels-last rows.

  max pool forward      nn.MaxPool2d(k, stride, (k - 1) // 2): scan the window in (dy, dx) order, skipping taps outside the map, and take
                        a tap when `val > max or isnan(val)` or it is the first one: the FIRST maximum, the LAST NaN, the window's first
                        tap when everything is -inf.  code = dy * k + dx (uint8; at most 14 * 15 + 14 = 224).  No arithmetic: values and
                        codes are exact, compared bit for bit (NaN as NaN), -0.0 and +0.0 told apart.  A map smaller than the unpadded
                        part of the window (n + 2 pad - k < 0) has no output; torch refuses it.
  max pool backward     dx[i] = sum of the g[o] whose code points at i (+ old): n terms and the accumulate term summed in fp32 in any
                        order, e = gamma(n - 1 + acc) (sum |g| + |old|), then stored().  n == 0 without accumulate: exactly 0.
  upsample forward      out[2y + i, 2x + j] = in[y, x]: a copy, bit for bit.
  upsample backward     four terms (+ old): e = gamma(3 + acc) (sum |t| + |old|), stored().
  axpby                 out = sa a + sb b (+ old), sa = alpha p0, sb = beta p1 in fp32.  Roundings on the path of the a term: sa (when
                        p0 is there), the product (none when sa is +-1), the add of the b term (when b is there), the accumulate;
                        of the b term: sb (when p1 is there), the product (absorbed when fused: counted), the add, the accumulate; of
                        old: the accumulate.  e = gamma(ra) |ta| + gamma(rb) |tb| + u |old|, stored().  alpha == 0: the a term is an
                        exact zero whatever `a` holds.  The `out` of dot is the same with b absent.
  dot                   red += sum a b: per thread a chain of EPV * trips multiply-adds (fused or not: one more rounding), the 6-step
                        wave fold, the 4-wave fold; one fp64 atomic per workgroup.  e = gamma(m) sum |a b| + 2^-53 G sum |a b|,
                        m = EPV * trips + 1 + 6 + 3, G workgroups.
  se_pool               pooled = alpha sum_p x (x y with `b`): per thread ceil(chunk / PY) terms, PY lane sums folded in turn, HS planes
                        folded in turn, alpha: m = ceil(chunk / PY) + PY + HS + 1, e = gamma(m) |alpha| sum |x|  (gamma(m + 1), sum
                        |x y| with `b`: the fp32 product).
  SE FC forward         h = relu(W1 pooled + b1), t2 = W2 h + b2, scale = clamp(t2 + 3, 0, 6) / 6.  A dot product of K terms plus the
                        bias in any association: e_t = gamma(K + 2) (sum |w v| + |b|).  relu and the clamp have slope <= 1: e_h = e_t.
                        scale: the add of 3, the rounded constant 1/6f, the product: e_s = (e_t + u |t2 + 3|) / 6 + 2 u |s|.
                        Each stage is held to ITS inputs: h to pooled, t2 and scale to the h the device stored.
  SE FC backward        dt2 = (-3 < t2 < 3) dscale / 6 (strict: 0 at t2 = +-3), two roundings (1/6f, the product);
                        dt1[j] = (h[j] > 0) sum_c W2[c][j] dt2[c]:  e = gamma(C + 4) sum |w dt2|;
                        dpooled[c] = sum_j W1[j][c] dt1[j] from the dt1 the device stored:  e = gamma(Cs + 2) sum |w dt1|;
                        dW2 += sum_b dt2 h, db2 += sum_b dt2:  e = gamma(B + 3) sum |.| + u |old + sum|;
                        dW1 += sum_b dt1 pooled, db1 += sum_b dt1:  e = gamma(B + 1) sum |.| + u |old + sum|.
  se_scale              out = a p0[b, c] + p1[b, c] alpha (+ old): p1 alpha, the product, the add (fused or not), the accumulate:
                        e = gamma(3 + acc) (|a p0| + |p1 alpha| + |old|), stored().
  se_scale, the reduce  see se_reduce().
  head permute          forward a copy; backward round-to-nearest-even of the fp32 gradient into the storage type, exact zeros in
                        the channels >= na * no; bias gradient db[c] += sum dp: per thread at most B ceil(cells / 1024) terms, then
                        (s0 + s1) + (s2 + s3), the wave fold, 16 wave sums, the +=: m = B ceil(cells / 1024) + 2 + 6 + 16 + 1,
                        e = gamma(m) (sum |dp| + |old|).
  weighted-fusion weights   weff = sigmoid(w) 2 / n and dw += red (2 / n) s (1 - s) through __expf, whose error is MEASURED, not derived:
                        see EXPF_ULPS below and DESIGN.md ("Elementwise kernels against fp64").
"""
import torch

from oracle.dwconv import F16_MAX, U, check, store, ulp  # noqa: F401
from oracle.stem import _stored as stored  # noqa: F401  (half an ulp of the storage type at |ref| + e: one definition)

_F64 = torch.float64
U64 = 2.0 ** -53


def gamma(n):
    n = torch.as_tensor(n, dtype=_F64)
    return n * U / (1.0 - n * U)


def check_nan(got, ref, bound):
    """check() where the reference may hold NaN: exactly those elements must be NaN, the others are held to their bound"""
    got, ref = got.to(_F64), ref.to(_F64)
    nan = torch.isnan(ref)
    wrong = int((torch.isnan(got) != nan).sum())
    z = torch.zeros_like(ref)
    ratio, bad = check(torch.where(nan, z, got), torch.where(nan, z, ref), torch.where(nan, z, bound.to(_F64)))
    return ratio, bad + wrong


def same_bits(got, want):
    """number of elements whose bits differ (a NaN equals any NaN); both of one dtype"""
    assert got.dtype == want.dtype and got.shape == want.shape
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    diff = got.contiguous().view(view) != want.contiguous().view(view)
    if got.is_floating_point():
        diff &= ~(torch.isnan(got) & torch.isnan(want))
    return int(diff.sum())


# ---------------------------------------------------------------------------------------------------- max pool
def pool_out(n, k, stride):
    m = n + 2 * ((k - 1) // 2) - k
    return 0 if m < 0 else m // stride + 1


def pool_fwd(x, k, stride=1):
    """(values [B, C, Ho, Wo], codes uint8) by the scan rule above.  x of any float dtype; there is no arithmetic, so a 16- or 32-bit
    input is scanned as float32 (every value exact) and the values come back in that type"""
    x = x if x.dtype == _F64 else x.float()
    B, C, H, W = x.shape
    pad = (k - 1) // 2
    Ho, Wo = pool_out(H, k, stride), pool_out(W, k, stride)
    assert Ho > 0 and Wo > 0
    ye, xe = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1
    ph, pw = max(0, ye + k - 1 - pad - H), max(0, xe + k - 1 - pad - W)
    xp = torch.nn.functional.pad(x, (pad, pw, pad, ph))
    vp = torch.nn.functional.pad(torch.ones(1, 1, H, W, dtype=torch.bool), (pad, pw, pad, ph))
    m = torch.full((B, C, Ho, Wo), float("-inf"), dtype=x.dtype)
    code = torch.zeros(B, C, Ho, Wo, dtype=torch.uint8)
    seen = torch.zeros(1, 1, Ho, Wo, dtype=torch.bool)
    for dy in range(k):
        for dx in range(k):
            tap = xp[:, :, dy:dy + ye:stride, dx:dx + xe:stride]
            ok = vp[:, :, dy:dy + ye:stride, dx:dx + xe:stride]
            take = ok & (~seen | (tap > m) | torch.isnan(tap))
            m = torch.where(take, tap, m)
            code = torch.where(take, torch.full_like(code, dy * k + dx), code)
            seen = seen | ok
    assert bool(seen.all())
    return m, code


def code_index(code, k, stride, H, W):
    """the flat input index ih * W + iw (torch's return_indices) a code stands for at its output position"""
    pad = (k - 1) // 2
    Ho, Wo = code.shape[2:]
    c = code.long()
    ih = torch.arange(Ho).view(1, 1, Ho, 1) * stride - pad + c // k
    iw = torch.arange(Wo).view(1, 1, 1, Wo) * stride - pad + c % k
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all())
    return ih * W + iw


def pool_bwd(g, code, k, stride, H, W, dtype, old=None):
    """(target, bound): the gather by the ORACLE's codes; a NaN gradient reaches exactly the input its output selected"""
    B, C = g.shape[:2]
    idx = code_index(code, k, stride, H, W).view(B, C, -1)
    g = g.to(_F64).reshape(B, C, -1)
    z = torch.zeros(B, C, H * W, dtype=_F64)
    s = z.clone().scatter_add_(2, idx, g)
    sa = z.clone().scatter_add_(2, idx, g.abs())
    n = z.clone().scatter_add_(2, idx, torch.ones_like(g))
    acc = 0
    if old is not None:
        o = old.to(_F64).reshape(B, C, -1)
        s, sa, acc = s + o, sa + o.abs(), 1
    e = gamma((n - 1 + acc).clamp(min=0)) * sa
    e = torch.where(torch.isnan(e), torch.zeros_like(e), e)
    tgt, b = stored(s, e, dtype)
    b = torch.where(torch.isnan(tgt), torch.zeros_like(b), b)
    if old is None:
        b = torch.where(n == 0, torch.zeros_like(b), b)
    return tgt.view(B, C, H, W), b.view(B, C, H, W)


# ---------------------------------------------------------------------------------------------------- upsample
def up_fwd(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def up_bwd(g, dtype, old=None):
    g = g.to(_F64)
    t = [g[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    s, sa, acc = sum(t), sum(v.abs() for v in t), 0
    if old is not None:
        s, sa, acc = s + old.to(_F64), sa + old.to(_F64).abs(), 1
    return stored(s, gamma(3 + acc) * sa, dtype)


# ---------------------------------------------------------------------------------------------------- axpby / dot
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def axpby(a, dtype, alpha=1.0, beta=1.0, b=None, p0=None, p1=None, old=None):
    """(target, bound).  a, b, old: tensors of one shape holding storage-type values; alpha, beta, p0, p1 fp32 scalars (p0 / p1 None: absent)"""
    alpha, beta = _f32(alpha), _f32(beta)
    sa = alpha * (1.0 if p0 is None else _f32(p0))
    sb = beta * (1.0 if p1 is None else _f32(p1))
    acc = 0 if old is None else 1
    if alpha == 0.0:
        ta, ra = torch.zeros(a.shape, dtype=_F64), 0
    else:
        ta = sa * a.to(_F64)
        ra = (p0 is not None) + (abs(_f32(sa)) != 1.0) + (b is not None) + acc
    tgt, e = ta, gamma(ra) * ta.abs()
    if b is not None:
        tb = sb * b.to(_F64)
        tgt, e = tgt + tb, e + gamma((p1 is not None) + 2 + acc) * tb.abs()
    if old is not None:
        tgt, e = tgt + old.to(_F64), e + U * old.to(_F64).abs()
    return stored(tgt, e, dtype)


def dot(a, b, epv, trips, grid):
    """(target, bound) of what one launch adds to red[0]"""
    p = a.to(_F64) * b.to(_F64)
    A = float(p.abs().sum())
    return p.sum(), float(gamma(epv * trips + 1 + 6 + 3)) * A + U64 * grid * A


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
def se_pool(x, alpha, m, y=None):
    """(target, bound) [B, C]; m = ceil(chunk / PY) + PY + HS + 1 from the launch geometry"""
    x = x.to(_F64)
    if y is not None:
        x, m = x * y.to(_F64), m + 1
    alpha = _f32(alpha)
    return alpha * x.sum((2, 3)), gamma(m) * abs(alpha) * x.abs().sum((2, 3))


def _matvec(W, v, bias=None):
    """(W v + bias, sum |w v| + |bias|): W [R, K], v [B, K] -> [B, R]"""
    W, v = W.to(_F64), v.to(_F64)
    t, A = v @ W.t(), v.abs() @ W.abs().t()
    if bias is not None:
        t, A = t + bias.to(_F64), A + bias.to(_F64).abs()
    return t, A


def se_fc1(pooled, w1, b1):
    """(target, bound) of h [B, Cs]"""
    t, A = _matvec(w1, pooled, b1)
    return t.clamp(min=0.0), gamma(w1.shape[1] + 2) * A


def se_fc2(h, w2, b2):
    """((t2, bound), (scale, bound)) [B, C] from the h the device stored"""
    t, A = _matvec(w2, h, b2)
    e_t = gamma(w2.shape[1] + 2) * A
    s = (t + 3.0).clamp(0.0, 6.0) / 6.0
    return (t, e_t), (s, (e_t + U * (t + 3.0).abs()) / 6.0 + 2 * U * s)


def se_dt2(t2, dscale):
    t2, dscale = t2.to(_F64), dscale.to(_F64)
    return torch.where((t2 > -3.0) & (t2 < 3.0), dscale / 6.0, torch.zeros_like(t2))


def se_dt1(h, t2, dscale, w2):
    """(target, bound) of dt1 [B, Cs]"""
    t, A = _matvec(w2.t(), se_dt2(t2, dscale))
    live = h.to(_F64) > 0
    z = torch.zeros_like(t)
    return torch.where(live, t, z), torch.where(live, gamma(w2.shape[0] + 4) * A, z)


def se_dpooled(dt1, w1):
    """(target, bound) of dpooled [B, C] from the dt1 the device stored"""
    t, A = _matvec(w1.t(), dt1)
    return t, gamma(w1.shape[0] + 2) * A


def _outer(v, o, old, extra):
    """old + sum_b v[b, r] o[b, c]: (target, bound)"""
    v, o = v.to(_F64), o.to(_F64)
    tgt = old.to(_F64) + v.t() @ o
    return tgt, gamma(v.shape[0] + extra) * (v.abs().t() @ o.abs()) + U * tgt.abs()


def se_wgrad(pooled, h, dt1, t2, dscale, old):
    """{dw1, db1, dw2, db2: (target, bound)}; h, dt1, t2 as the workspace holds them; old: the four initial tensors"""
    dt2 = se_dt2(t2, dscale)
    ones = torch.ones(h.shape[0], 1, dtype=_F64)
    res = {"dw2": _outer(dt2, h, old["dw2"], 3), "dw1": _outer(dt1, pooled, old["dw1"], 1)}
    for nm, v, extra in (("db2", dt2, 3), ("db1", dt1, 1)):
        t, b = _outer(v, ones, old[nm].view(-1, 1), extra)
        res[nm] = (t.view(-1), b.view(-1))
    return res


def se_scale(a, p0, dtype, p1=None, alpha=1.0, old=None):
    """(target, bound); a, old [B, C, H, W], p0, p1 [B, C]"""
    v = lambda t: t.to(_F64)[:, :, None, None]
    ta = a.to(_F64) * v(p0)
    tgt, A, acc = ta, ta.abs(), 0
    if p1 is not None:
        tb = v(p1) * _f32(alpha)
        tgt, A = tgt + tb, A + tb.abs()
    if old is not None:
        tgt, A, acc = tgt + old.to(_F64), A + old.to(_F64).abs(), 1
    return stored(tgt, gamma(3 + acc) * A, dtype)


# activation -> (derivative in fp64, [(kink, jump of the derivative there)], own evaluation error of the derivative given (t, e_t))
def _mish_d(t):
    th = torch.tanh(torch.nn.functional.softplus(t, threshold=40.0))
    return th + t * (1 - th * th) * torch.sigmoid(t)


def _mish_err(t, e_t):
    """act_bwd writes mish' = [n (n + 2) + 4 t e (e + 1)] / (n + 2)^2, n = e (e + 2), e = __expf(min(t, 20)).  With the exponential's
    relative error taken as in oracle/stem.py (argument scaling |t| u, one ulp of v_exp_f32: eps = (|t| + 2) u) both positive quotients
    P = n / (n + 2) and Q = 4 |t| e (e + 1) / (n + 2)^2 move by at most 6 eps, ten roundings and one ulp of v_rcp_f32 on top; |mish''| < 1.1"""
    e = torch.exp(t.clamp(max=20.0))
    n = e * (e + 2)
    PQ = n / (n + 2) + 4 * t.abs() * e * (e + 1) / (n + 2) ** 2
    return PQ * (6 * (t.abs() + 2) + 11) * U + 1.1 * e_t


_ACT_D = {
    "linear": (lambda t: torch.ones_like(t), [], lambda t, e_t: torch.zeros_like(t)),
    "leaky": (lambda t: torch.where(t > 0, 1.0, 0.1).to(_F64), [(0.0, 0.9)], lambda t, e_t: torch.full_like(t, U)),
    "relu": (lambda t: (t > 0).to(_F64), [(0.0, 1.0)], lambda t, e_t: torch.zeros_like(t)),
    "relu6": (lambda t: ((t > 0) & (t < 6)).to(_F64), [(0.0, 1.0), (6.0, 1.0)], lambda t, e_t: torch.zeros_like(t)),
    "hard-swish": (lambda t: torch.where(t < -3, 0.0, torch.where(t <= 3, t / 3 + 0.5, 1.0)).to(_F64), [(-3.0, 0.5), (3.0, 0.5)],
                   lambda t, e_t: torch.where(t.abs() <= 3 + e_t, e_t / 3 + 2 * U * (t.abs() / 3 + 0.5), torch.zeros_like(t))),
    "mish": (_mish_d, [], _mish_err),
    # (x > -3 && x < 3) ? 1 / 6f : 0 -- strict on both sides, the rounded constant
    "hard-sigmoid": (lambda t: ((t > -3) & (t < 3)).to(_F64) / 6.0, [(-3.0, 1.0 / 6.0), (3.0, 1.0 / 6.0)], lambda t, e_t: torch.full_like(t, U / 6.0)),
}
REDUCE_ACTS = ["linear", "leaky", "relu", "relu6", "hard-swish", "mish"]      # what the reduce riding on dyk_se_scale is run with


def se_reduce(g, yraw, vecs, act, m):
    """the BatchNorm-backward sums that ride on dyk_se_scale: (S [2, C], bound [2, C]).  g: the gradient the launch STORED (read back: the
    kernel forms the sums from the rounded value), yraw the producer's raw output, vecs = scale | shift | mean | rstd [4, C].
        t = yraw scale + shift (fp32, fused or not: e_t = 2u (|yraw scale| + |shift|)),  da = g act'(t),  xhat = (yraw - mean) rstd
        S1 = sum da,  S2 = sum da xhat            over images and pixels, per channel
    Per element: da is off by |g| (e_act + u |act'|) (the derivative's own error, the product); where t lies within e_t of a kink of
    the derivative either side may be taken: |g| times the jump more.  da xhat: three more roundings.  The sums: per-thread fp32 chains
    and the lane fold, m roundings in all (restated launch geometry), then fp64 atomics."""
    d, kinks, err = _ACT_D[act]
    v = lambda i: vecs[i].to(_F64).view(1, -1, 1, 1)
    g, y = g.to(_F64), yraw.to(_F64)
    t = y * v(0) + v(1)
    e_t = 2 * U * ((y * v(0)).abs() + v(1).abs())
    a = d(t)
    e_a = err(t, e_t) + U * a.abs()
    for kink, jump in kinks:
        e_a = e_a + jump * ((t - kink).abs() <= e_t).to(_F64)
    da, e_da = g * a, g.abs() * e_a
    xhat = (y - v(2)) * v(3)
    dx = da * xhat
    S = torch.stack([da.sum((0, 2, 3)), dx.sum((0, 2, 3))])
    b1 = e_da.sum((0, 2, 3)) + gamma(m) * da.abs().sum((0, 2, 3))
    b2 = (e_da * xhat.abs() + 3 * U * dx.abs()).sum((0, 2, 3)) + gamma(m) * dx.abs().sum((0, 2, 3))
    return S, torch.stack([b1, b2])


# ---------------------------------------------------------------------------------------------------- head
def head_fwd(y, na, no):
    """y [B, ny, nx, na*no] -> p [B, na, ny, nx, no]"""
    B, ny, nx, _ = y.shape
    return y.view(B, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous()


def head_bwd(dp, ld, dtype):
    """dp [B, na, ny, nx, no] fp32 -> dy [B, ny, nx, ld] of `dtype`, exactly"""
    B, na, ny, nx, no = dp.shape
    dy = torch.zeros(B, ny, nx, ld, dtype=dtype)
    dy[..., :na * no] = dp.permute(0, 2, 3, 1, 4).reshape(B, ny, nx, na * no).to(dtype)
    return dy


def head_bias(dp, old):
    B, na, ny, nx, no = dp.shape
    d = dp.to(_F64).permute(1, 4, 0, 2, 3).reshape(na * no, -1)
    m = B * (-(-ny * nx // 1024)) + 2 + 6 + 16 + 1
    tgt = old.to(_F64) + d.sum(1)
    return tgt, gamma(m) * (d.abs().sum(1) + old.to(_F64).abs())


# ---------------------------------------------------------------------------------------------------- weighted-fusion weights
# sigmoid(w) = 1 / (1 + __expf(-w)): the error of __expf is not derived here.  Measured on an MI355X over w in [-12, 12] (4096 points,
# n = 64 so that 2 / n is exact): the largest error of weff is 13.65 u |ref| (at w = -11.18; mean 1.46).  The bound is four times that,
# rounded up to a power of two; the margin covers inputs between the sampled points.
EXPF_MEASURED = 13.6531
EXPF_ULPS = 64.0
WFUSE_RANGE = 12.0


def wfuse_weights(w):
    """(target, bound) of weff = sigmoid(w) * (2 / n), |w| <= 12: the measured sigmoid figure, the rounded 2 / n and the product"""
    w = w.to(_F64)
    assert float(w.abs().max()) <= WFUSE_RANGE
    ref = torch.sigmoid(w) * (2.0 / w.numel())
    return ref, (EXPF_ULPS + 2) * U * ref.abs()


def wfuse_bwd(w, red, old):
    """(target, bound) of dw = old + fp32(red) * (2 / n) * s * (1 - s): s within EXPF_ULPS u s, so s (1 - s) within |1 - 2 s| of that;
    the conversion of red, 2 / n, 1 - s and the three products: 6 roundings (7 with second-order terms); the +="""
    w, red = w.to(_F64), red.to(_F64)
    assert float(w.abs().max()) <= WFUSE_RANGE
    s = torch.sigmoid(w)
    f = red * (2.0 / w.numel())
    tgt = old.to(_F64) + f * s * (1 - s)
    return tgt, f.abs() * U * (EXPF_ULPS * s * (1 - 2 * s).abs() + 7 * s * (1 - s)) + U * tgt.abs()
