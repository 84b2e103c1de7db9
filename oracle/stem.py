"""fp64 restatement of the Cin = 3 stem convolution (csrc/stem.hip: dyk_stem_conv_fwd / dyk_stem_conv_wgrad; `imgs.float() / 255.0`
of reference train_utils/kaist_train_eval_utils.py:54-55 followed by nn.Conv2d(3, C, 3, padding=1) of models.py:34-42, and that
layer's weight gradient) and DERIVED per-element bounds on what an fp32 evaluation of the same sums, stored in fp32, bf16 or fp16,
may differ by.  Plain torch on the CPU; no bound is tuned against a kernel and none depends on which kernel ran.

Inputs: image [B, 3, H, W], uint8 or fp32; w [Cout, 27] in the parameter-store order [co][ky][kx][c] (the kernels take its
[27][Cout] transpose); dy [B, Cout, Ho, Wo] already rounded to the storage type.  A uint8 image enters as x = fp32(p) / 255.0
evaluated in fp32 (the reference project's expression); that x is then taken as exact.

    patch[b, tc, yo, xo] = x[b, c, yo*s - 1 + ky, xo*s - 1 + kx]      tc = (ky*3 + kx)*3 + c, zero outside the image
    y  = sum_tc patch * w[co, tc]            A_y  = sum_tc |patch| |w|
    S1 = sum y, S2 = sum y^2 per filter      n    = B * Ho * Wo
    dw[co, tc] = sum_p dy * patch            A_dw = sum_p |dy * patch|

Bounds, u = 2^-24.

  forward accumulator   e = 88 u A_y.  The scalar kernel: 27 fma, at most 2*27 u A.  The MFMA kernel: products of an 8-bit pixel
                        with an 8-bit weight term are exact, the three truncated terms have the sign of w (|hi| + |mid| + |lo| = |w|),
                        which leaves 81 fp32 additions, the rounded constant 1/255f, the final product and the reference's own
                        rounding of p / 255: (81 + 4) u A, rounded up to 88.
  stored element        fp32: |got - y| <= e.  bf16 / fp16: e + ulp_T(|y| + e) / 2; fp16 clamps at +-65504 first.
  statistics            from the fp32 accumulators (error e each), fp32 partial sums of at most n terms, the replicas in fp64:
                        |s1 - S1| <= sum e + n u sum|y|,  |s2 - S2| <= sum (2|y|e + e^2 + u y^2) + n u sum y^2
  eval epilogue         z = act(t), t = y*scale + shift:  e_t = |scale| e + 2u (|y*scale| + |shift|),  e_z = L_act e_t + a_act
                        L_act the largest slope (1 linear, leaky, relu6; 1.5 hard-swish; 1.09 mish), a_act the activation's own
                        evaluation error: 0 linear and relu6, u|z| leaky, 4u|z| hard-swish (relu and hard-sigmoid, which the stem's
                        cases do not run: see the table below and oracle/bn_act.py), and for mish as act_fwd writes it
                        (e = __expf(min(t, 20)), n = e (e + 2), t * n * rcp(n + 2))  a_act = (2 (|t| + 4) + 4) u |z|: the argument
                        scaling of the exponential, |t| u, plus 1 ulp each for v_exp_f32 and v_rcp_f32 carried through n / (n + 2).
                        Then the storage rule with e_z.
  weight gradient       |dw - (old + DW)| <= (n + 4) u A_dw + u |old + DW|: n products and n additions in fp32 in any order,
                        planes folded in fp32, the uint8 kernel's single 1/255 behind the sum, the final dw +=.
  exact field           dy in {-1, 0, 1}, pixels 0..15 (a uint8 image, or a float image p / 256), sum |dy| p < 2^24 per element:
                        every fp32 sum is exact in any order and the bound shrinks to u A_dw + 3u |DW| + u |old + DW|.  Valid for
                        a float image on any kernel; for a uint8 image only where the sum-then-scale kernel runs.
  fused BatchNorm-backward apply   target DW* = sum_p bf16(dz_p) patch_p, dz = sc (da - S1/N - xhat S2/N) in fp64,
                        xhat = (yraw - mean) rstd.  The kernel's fp32 dz is within e_dz = 8u |sc| (|da| + |S1/N| + |xhat||S2/N|).  An
                        element whose fp64 dz lies within e_dz of a bf16 rounding midpoint is AMBIGUOUS: its stored value may be
                        either neighbour.  Bound: the weight-gradient bound + sum over ambiguous p of ulp_bf16(dz_p) |patch_p|;
                        condition: at most 1 % of the (pixel, filter) pairs are ambiguous.
                        dgamma / dbeta: |got - (old + S)| <= u|S| + u|old + S|.
"""
import torch

from oracle.dwconv import F16_MAX, U, check, store, ulp  # noqa: F401  (store, ulp, check: one definition for both suites)

_F64 = torch.float64
ACC_ULPS = 88.0
AMBIGUOUS_SHARE = 0.01

# activation -> (largest slope, own evaluation error as a function of (t, z) in units of u).  The one table of the forward activations: the
# stem suite runs ACTS, the BatchNorm/activation suite (oracle/bn_act.py) all seven.  relu is a selection (no arithmetic); hard-sigmoid
# is fminf(fmaxf(t + 3, 0), 6) * (1 / 6f): the add (u |t + 3|, carried through the slope 1/6), the rounded constant and the product.
_ACT = {
    "linear": (1.0, lambda t, z: torch.zeros_like(z)),
    "leaky": (1.0, lambda t, z: z.abs()),
    "relu6": (1.0, lambda t, z: torch.zeros_like(z)),
    "hard-swish": (1.5, lambda t, z: 4.0 * z.abs()),
    "mish": (1.09, lambda t, z: (2.0 * (t.abs() + 4.0) + 4.0) * z.abs()),
    "relu": (1.0, lambda t, z: torch.zeros_like(z)),
    "hard-sigmoid": (1.0 / 6.0, lambda t, z: (t + 3.0).abs() / 6.0 + 2.0 * z.abs()),
}
ACTS = ["linear", "leaky", "relu6", "hard-swish", "mish"]          # what the stem's eval epilogue is run with
ALL_ACTS = list(_ACT)


def act64(name, t):
    F = torch.nn.functional
    if name == "linear":
        return t
    if name == "leaky":
        return torch.where(t > 0, t, 0.1 * t)
    if name == "relu6":
        return t.clamp(0.0, 6.0)
    if name == "relu":
        return t.clamp(min=0.0)
    if name == "hard-sigmoid":
        return (t + 3.0).clamp(0.0, 6.0) / 6.0
    if name == "hard-swish":
        return t * (t + 3.0).clamp(0.0, 6.0) / 6.0
    if name == "mish":
        return t * torch.tanh(F.softplus(t, threshold=40.0))
    raise KeyError(name)


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def image_values(img):
    """the convolution's input as fp64: a uint8 image as fp32(p) / 255.0 evaluated in fp32"""
    if img.dtype == torch.uint8:
        return (img.float() / 255.0).to(_F64)
    assert img.dtype == torch.float32
    return img.to(_F64)


def patches(x, stride):
    """[B, 27, Ho, Wo], tc = (ky*3 + kx)*3 + c, zero outside the image; the dtype of x"""
    B, C, H, W = x.shape
    assert C == 3
    Ho, Wo = out_hw(H, W, stride)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    ye, xe = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1
    out = x.new_empty(B, 27, Ho, Wo)
    for ky in range(3):
        for kx in range(3):
            out[:, (ky * 3 + kx) * 3:(ky * 3 + kx) * 3 + 3] = xp[:, :, ky:ky + ye:stride, kx:kx + xe:stride]
    return out


class Reference:
    """fp64 quantities of one problem: P (patches), y, A_y, S1, S2, n; with dy also dw, A_dw [Cout, 27]"""


def reference(img, w, stride, dy=None, forward=True):
    r = Reference()
    r.stride = stride
    r.P = patches(image_values(img), stride)
    B, _, Ho, Wo = r.P.shape
    r.n = B * Ho * Wo
    if forward:
        w = w.to(_F64)
        assert w.shape[1] == 27
        r.y = torch.einsum("ot,btyx->boyx", w, r.P)
        r.A_y = torch.einsum("ot,btyx->boyx", w.abs(), r.P.abs())
        r.S1, r.S2 = r.y.sum((0, 2, 3)), (r.y * r.y).sum((0, 2, 3))
    if dy is not None:
        r.dw, r.A_dw = weight_gradient(r.P, dy)
    return r


def weight_gradient(P, dy):
    dy = dy.to(_F64)
    assert dy.shape[0] == P.shape[0] and dy.shape[2:] == P.shape[2:]
    return torch.einsum("boyx,btyx->ot", dy, P), torch.einsum("boyx,btyx->ot", dy.abs(), P.abs())


# ---------------------------------------------------------------------------------------------------- forward
def acc_error(A):
    return ACC_ULPS * U * A


def _stored(tgt, e, dtype):
    if dtype == torch.float32:
        return tgt, e
    if dtype == torch.float16:
        tgt = tgt.clamp(-F16_MAX, F16_MAX)
    return tgt, e + 0.5 * ulp(tgt.abs() + e, dtype)


def out_bound(r, dtype):
    """(target, bound) of a stored raw forward element"""
    return _stored(r.y, acc_error(r.A_y), dtype)


def stats_bound(r):
    """the stats_bound formulas of oracle/dwconv.py with this module's e"""
    e, y = acc_error(r.A_y), r.y
    b1 = e.sum((0, 2, 3)) + r.n * U * y.abs().sum((0, 2, 3))
    b2 = (2 * y.abs() * e + e * e + U * y * y).sum((0, 2, 3)) + r.n * U * (y * y).sum((0, 2, 3))
    return b1, b2


def affine_bound(r, scale, shift, act, dtype):
    """(target, bound) of a stored element of the eval epilogue z = act(y * scale + shift)"""
    L_act, a_act = _ACT[act]
    sc, sh = scale.to(_F64).view(1, -1, 1, 1), shift.to(_F64).view(1, -1, 1, 1)
    t = r.y * sc + sh
    z = act64(act, t)
    e_t = sc.abs() * acc_error(r.A_y) + 2 * U * ((r.y * sc).abs() + sh.abs())
    e_z = L_act * e_t + U * a_act(t, z)
    return _stored(z, e_z, dtype)


# ---------------------------------------------------------------------------------------------------- weight gradient
def dw_bound(n, dw, A_dw, old=None):
    """(target, bound): fp32 products and sums in any order, planes folded in fp32, one 1/255 behind the sum, the final +="""
    tgt = dw if old is None else dw + old.to(_F64)
    return tgt, (n + 4) * U * A_dw + U * tgt.abs()


def dw_bound_exact(dw, A_dw, old=None):
    """(target, bound) on the exact field: every fp32 sum is exact; what is left is the reference's rounding of p / 255, the 1/255f
    behind the sum and the final +="""
    tgt = dw if old is None else dw + old.to(_F64)
    return tgt, U * A_dw + 3 * U * dw.abs() + U * tgt.abs()


def assert_exact_field(img, dy, stride):
    """dy in {-1, 0, 1}, pixel values p in 0..15 (uint8, or float p / 256), sum |dy| p < 2^24 for every (filter, patch element)"""
    p = img.to(_F64) if img.dtype == torch.uint8 else img.to(_F64) * 256.0
    assert bool((p == p.round()).all()) and float(p.min()) >= 0 and float(p.max()) <= 15
    d = dy.to(_F64)
    assert bool(((d == 0) | (d.abs() == 1)).all())
    tot = torch.einsum("boyx,btyx->ot", d.abs(), patches(p, stride))
    assert float(tot.max()) < 2.0 ** 24


# ---------------------------------------------------------------------------------------------------- fused BatchNorm-backward apply
class Fused:
    """dz64, dzb (its bf16 rounding as fp64), e_dz, ambiguous (bool), share, S1, S2 (the folded replicas) of one fused problem"""


def fused_reference(da, yraw, scale, mean, rstd, red):
    """da, yraw [B, C, Ho, Wo] (bf16 values); scale, mean, rstd [C] fp32; red [slots, 2, C] fp64 (sum da, sum da * xhat)"""
    f = Fused()
    v = lambda t: t.to(_F64).view(1, -1, 1, 1)
    da, yraw = da.to(_F64), yraw.to(_F64)
    N = da.shape[0] * da.shape[2] * da.shape[3]
    f.S1, f.S2 = red[:, 0].to(_F64).sum(0), red[:, 1].to(_F64).sum(0)
    m1, m2 = v(f.S1) / N, v(f.S2) / N
    xhat = (yraw - v(mean)) * v(rstd)
    f.dz64 = v(scale) * (da - m1 - xhat * m2)
    f.e_dz = 8 * U * v(scale).abs() * (da.abs() + m1.abs() + xhat.abs() * m2.abs())
    f.dzb = f.dz64.float().bfloat16().to(_F64)
    # distance of |dz| to the nearest rounding midpoint (k + 1/2) q of the bf16 grid around it
    a = f.dz64.abs()
    dist = None
    for q in (ulp(a, torch.bfloat16), ulp(a + f.e_dz, torch.bfloat16), ulp((a - f.e_dz).clamp(min=0), torch.bfloat16)):
        dq = ((a / q) % 1.0 - 0.5).abs() * q
        dist = dq if dist is None else torch.minimum(dist, dq)
    f.ambiguous = dist <= f.e_dz
    f.share = float(f.ambiguous.double().mean())
    return f


def fused_dw_bound(f, P, n, old=None):
    """(target, bound) of the fused weight gradient; asserts nothing: the caller checks f.share <= AMBIGUOUS_SHARE"""
    dw, A_dw = weight_gradient(P, f.dzb)
    tgt, b = dw_bound(n, dw, A_dw, old)
    slack = ulp(f.dz64, torch.bfloat16) * f.ambiguous.to(_F64)
    return tgt, b + torch.einsum("boyx,btyx->ot", slack, P.abs())


def sum_bound(S, old):
    """(target, bound) of dgamma / dbeta: old + fp32(S)"""
    tgt = S.to(_F64) + old.to(_F64)
    return tgt, U * S.abs().to(_F64) + U * tgt.abs()
