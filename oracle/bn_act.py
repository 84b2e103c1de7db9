"""fp64 restatement of the BatchNorm/activation kernels of csrc/bn_act.hip (training-mode nn.BatchNorm2d followed by the activation of
reference models.py:34-62, its eval-mode fold, and the three backward passes) and DERIVED per-element bounds on what the kernels'
fp64 / fp32 evaluation, stored in fp32, bf16 or fp16, may differ by.  Plain torch on the CPU; no bound is tuned against a kernel.

Tensors are rows here: x [P, C] (P pixels of C channels, the kernels' channels-last view), per-channel vectors [C], statistics replicas
[slots, 2, C] in fp64.  u = 2^-24 (U), u64 = 2^-53 (U64), gamma(n) = n u / (1 - n u), stored() the storage rule of oracle/stem.py.
The activation tables are those of oracle/stem.py (_ACT: largest slope L_act and own evaluation error a_act of the forward) and
oracle/elementwise.py (_ACT_D: derivative, its kinks and jumps, own evaluation error): one definition per activation for every suite.

  finalize   S1, S2 = the sums of the replicas, taken here with math.fsum (correctly rounded).  The kernels fold them in fp64 in some
             order: e_S = slots u64 sum |s|.  mean = S1 / n: e_mean = e_S1 / n + u64 |mean|.  var = max(0, S2 / n - mean^2), the
             cancellation: e_var = 2 [e_S2 / n + u64 S2 / n + 2 |mean| e_mean + e_mean^2 + u64 mean^2 + u64 |var|] (the factor 2: this
             module's own fp64 evaluation of the same difference).  rstd = fp32(1 / sqrt(var + eps)), eps the fp32 value: e_var is
             carried through the function itself (evaluated at var -+ e_var, the lower end clamped at 0), 4 u64 rstd for sqrt, the add
             and the division, u rstd for the conversion.  scale = fp32(g rstd): |g| e_rstd + u |scale|.
             shift = b - fp32(mean) scale, fused or not: |scale| e_mean + |mean| e_scale + 2u |mean scale| + u |shift|.  Held to the
             values the launch itself stored (shift_given): b - save_mean scale is then off by u |mean scale| (the product, absent when
             fused) + u |shift| only, which is what tells a shift formed from the unrounded scale.
             running_mean = (1 - m) old + m fp32(mean): three roundings on either term, gamma(3) (|(1 - m) old| + |m mean|) + m e_mean;
             running_var the same with unb = var n / (n - 1) (n == 1: var), e_unb = (e_var + 3 u64 var) n / (n - 1).
  fold       scale = g / sqrtf(rv + eps): the add (u, halved by the root), sqrtf and the division to one ulp (2u each): 4.5 u |scale|;
             shift = b - rm scale: |rm| e_scale + u |rm scale| + u |shift|.  Null gamma: g = 1; null beta: b = 0.
  forward    z = act(t) (+ r), t = x sc + sh in fp32, fused or not: e_t = 2u (|x sc| + |sh|); e_t = 0 where sh == 0 and sc is a power of
             two (t is then exact).  e_z = L_act e_t + a_act, + u |z + r| with the residual, then stored(); fp16 clamps at +-65504 first.
             (leaky's a_act = u |z| is the product's rounding; the 0.25 u of the constant 0.1f sits in the slack of e_t, which is at
             least u |t| wide whenever it is not 0.)
  reduce     da = g act'(t), xhat = (y - mean) rstd, S1 = sum da, S2 = sum da xhat per channel.  da is off by |g| (e_act + u |act'|);
             where |t - kink| <= e_t either side of the derivative may be taken: |g| jump more.  da xhat: three more roundings.  The
             fp32 sums: a per-thread chain of chunk / PY terms and PY - 1 additions through LDS, m = chunk / PY + PY - 1 roundings
             (the launch geometry, restated by reduce_grid), then one fp64 atomic per workgroup: gy u64 sum |.| on top.  The test sums
             the replicas in fp64 on the host.
  params     replica 0 holds the totals afterwards: slots u64 sum |s|;  dgamma / dbeta: u |S| + u |old + S| (oracle/stem.py sum_bound)
             + the fold.
  apply      dy = sc (da - S1 / N - xhat S2 / N) (+ old), the totals from the replicas the test wrote (math.fsum):
             e = 8u |sc| (|da| + |S1 / N| + |xhat| |S2 / N|) + |sc| e_da (+ u |old + dy|), then stored().  8: the fp32 conversion of a
             total, 1 / N, their product, the two roundings of xhat, its product with S2 / N, the two subtractions, the product with sc.

ew_grid / reduce_grid restate the host's grid arithmetic (ew_grid2d and the body of dyk_bn_act_bwd_reduce) so that a case can assert
the path it claims.
"""
import collections
import math

import torch

from oracle.dwconv import F16_MAX, U, check, store, ulp  # noqa: F401
from oracle.elementwise import U64, _ACT_D, gamma, same_bits  # noqa: F401
from oracle.stem import _ACT, ALL_ACTS, act64, sum_bound  # noqa: F401
from oracle.stem import _stored as stored

_F64 = torch.float64
ACTS = ALL_ACTS                       # linear, leaky, relu6, hard-swish, mish, relu, hard-sigmoid
KINK_SHARE = 1e-3


def epv(dt):
    return 4 if dt == "f32" else 8


# ---------------------------------------------------------------------------------------------------- launch geometry
Grid = collections.namedtuple("Grid", "CV CVB PY gx gy chunk rows live empty last")


def _grid(C, npix, dt):
    CV = C // epv(dt)
    CVB = 1
    while CVB < CV and CVB < 32:
        CVB *= 2
    PY, gx = 256 // CVB, -(-CV // CVB)
    gy = max(1, min(-(-npix // (PY * 8)), max(1, 2048 // gx)))
    chunk = -(-(-(-npix // gy)) // PY) * PY
    live = -(-npix // chunk)
    return Grid(CV, CVB, PY, gx, gy, chunk, chunk // PY, live, gy - live, npix - (live - 1) * chunk)


def ew_grid(C, npix, dt):
    """ew_grid2d and the kernels' chunking: CV vectors in groups of CVB (power of two <= 32), PY = 256 / CVB pixel lanes, gx groups,
    gy = clamp(ceil(npix / 8 PY), 1, 2048 / gx) workgroups along the pixels, each a contiguous chunk (a multiple of PY) walked in
    `rows` rows per thread; `live` workgroups have pixels, `empty` have none, the last live one has `last`"""
    return _grid(C, npix, dt)


def reduce_grid(C, npix, dt):
    """the same arithmetic, written out a second time in dyk_bn_act_bwd_reduce"""
    return _grid(C, npix, dt)


def reduce_m(g):
    return g.rows + g.PY - 1


# ---------------------------------------------------------------------------------------------------- finalize / fold
def exact_sum(x):
    """[R, C] fp64 -> [C], correctly rounded"""
    return torch.tensor([math.fsum(col) for col in x.to(_F64).t().tolist()], dtype=_F64)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _vec(v, C, fill):
    return torch.full((C,), fill, dtype=_F64) if v is None else v.to(_F64)


def finalize(stats, count, eps, g=None, b=None, momentum=0.0, rm=None, rv=None):
    """{name: (target, bound)} of mean, rstd, scale, shift (and running_mean, running_var with rm / rv) from the replicas [slots, 2, C]"""
    st = stats.to(_F64)
    slots, _, C = st.shape
    n, eps, mom = float(count), _f32(eps), _f32(momentum)
    S1, S2 = exact_sum(st[:, 0]), exact_sum(st[:, 1])
    e1, e2 = slots * U64 * st[:, 0].abs().sum(0), slots * U64 * st[:, 1].abs().sum(0)
    mean = S1 / n
    e_mean = e1 / n + U64 * mean.abs()
    raw = S2 / n - mean * mean
    e_var = 2 * (e2 / n + U64 * (S2 / n).abs() + 2 * mean.abs() * e_mean + e_mean ** 2 + U64 * mean * mean + U64 * raw.abs())
    var = raw.clamp(min=0.0)
    r = (var + eps) ** -0.5
    r_hi, r_lo = ((var - e_var).clamp(min=0.0) + eps) ** -0.5, (var + e_var + eps) ** -0.5
    e_r = torch.maximum(r_hi - r, r - r_lo) + 4 * U64 * r + U * r
    gg, bb = _vec(g, C, 1.0), _vec(b, C, 0.0)
    sc = gg * r
    e_sc = gg.abs() * e_r + U * sc.abs()
    sh = bb - mean * sc
    e_sh = sc.abs() * e_mean + mean.abs() * e_sc + 2 * U * (mean * sc).abs() + U * sh.abs()
    out = {"mean": (mean, e_mean + U * mean.abs()), "rstd": (r, e_r), "scale": (sc, e_sc), "shift": (sh, e_sh), "var": (var, e_var),
           "raw_var": (raw, e_var)}
    if rm is not None:
        a, bm = (1.0 - mom) * rm.to(_F64), mom * mean
        out["running_mean"] = (a + bm, gamma(3) * (a.abs() + bm.abs()) + mom * e_mean)
        k = n / (n - 1.0) if n > 1 else 1.0
        unb, e_unb = var * k, (e_var + 3 * U64 * var) * k
        a, bv = (1.0 - mom) * rv.to(_F64), mom * unb
        out["running_var"] = (a + bv, gamma(3) * (a.abs() + bv.abs()) + mom * e_unb)
    return out


def shift_given(b, mean32, scale32):
    """(target, bound) of shift held to the save_mean and scale the launch stored"""
    p = mean32.to(_F64) * scale32.to(_F64)
    tgt = _vec(b, p.numel(), 0.0) - p
    return tgt, U * p.abs() + U * tgt.abs()


def fold(rm, rv, eps, g=None, b=None):
    """{scale, shift: (target, bound)} of the eval-mode fold"""
    C = rm.numel()
    sc = _vec(g, C, 1.0) / (rv.to(_F64) + _f32(eps)).sqrt()
    e_sc = 4.5 * U * sc.abs()
    p = rm.to(_F64) * sc
    sh = _vec(b, C, 0.0) - p
    return {"scale": (sc, e_sc), "shift": (sh, rm.to(_F64).abs() * e_sc + U * p.abs() + U * sh.abs())}


# ---------------------------------------------------------------------------------------------------- forward
def _pow2(v):
    m, _ = torch.frexp(v.abs())
    return m == 0.5


def preact(x, sc, sh):
    """(t, e_t) of t = x sc + sh in fp32, fused or not; x [P, C]; sc / sh [C] or None (1 / 0)"""
    x = x.to(_F64)
    C = x.shape[1]
    sc, sh = _vec(sc, C, 1.0), _vec(sh, C, 0.0)
    t = x * sc + sh
    e_t = 2 * U * ((x * sc).abs() + sh.abs())
    exact = ((sh == 0) & _pow2(sc)).view(1, -1)
    return t, torch.where(exact, torch.zeros_like(e_t), e_t)


def forward(x, sc, sh, act, dtype, r=None):
    """(target, bound) of a stored element of z = act(x sc + sh) (+ r)"""
    L_act, a_act = _ACT[act]
    t, e_t = preact(x, sc, sh)
    z = act64(act, t)
    e = L_act * e_t + U * a_act(t, z)
    if r is not None:
        z = z + r.to(_F64)
        e = e + U * z.abs()
    return stored(z, e, dtype)


# ---------------------------------------------------------------------------------------------------- backward
class DAct:
    """da, e_da, t, e_t, near (bool: within e_t of a kink of the derivative) of one problem"""


def dact(g, y, sc, sh, act):
    d, kinks, err = _ACT_D[act]
    r = DAct()
    r.t, r.e_t = preact(y, sc, sh)
    a = d(r.t)
    e_a = err(r.t, r.e_t) + U * a.abs()
    r.near = torch.zeros_like(r.t, dtype=torch.bool)
    for kink, jump in kinks:
        hit = ((r.t - kink).abs() <= r.e_t) & (r.e_t > 0)
        e_a = e_a + jump * hit.to(_F64)
        r.near |= hit
    g = g.to(_F64)
    r.da, r.e_da = g * a, g.abs() * e_a
    return r


def kink_share(y, sc, sh, act):
    return float(dact(torch.ones_like(y, dtype=_F64), y, sc, sh, act).near.double().mean())


def reduce(g, y, vecs, act, grid):
    """(S [2, C], bound [2, C]) of what one reduce launch adds to its replicas, summed over them; vecs = scale | shift | mean | rstd"""
    r = dact(g, y, vecs[0], vecs[1], act)
    xhat = (y.to(_F64) - vecs[2].to(_F64)) * vecs[3].to(_F64)
    dx = r.da * xhat
    m = gamma(reduce_m(grid)) + grid.gy * U64
    S = torch.stack([r.da.sum(0), dx.sum(0)])
    b1 = r.e_da.sum(0) + m * r.da.abs().sum(0)
    b2 = (r.e_da * xhat.abs() + 3 * U * dx.abs()).sum(0) + m * dx.abs().sum(0)
    return S, torch.stack([b1, b2])


def totals(red):
    """(S [2, C], fold bound [2, C]) of replicas [slots, 2, C]: math.fsum, and what an fp64 fold in any order may miss"""
    red = red.to(_F64)
    S = torch.stack([exact_sum(red[:, 0]), exact_sum(red[:, 1])])
    return S, red.shape[0] * U64 * red.abs().sum(0)


def param_bound(S, e_fold, old):
    """(target, bound) of dgamma / dbeta = old + fp32(S)"""
    tgt, b = sum_bound(S, old)
    return tgt, b + e_fold


def apply(g, y, vecs, act, S, npix, dtype, old=None):
    """(target, bound) of a stored element of dy; S [2, C] the totals of the replicas"""
    sc = vecs[0].to(_F64)
    r = dact(g, y, vecs[0], vecs[1], act)
    xhat = (y.to(_F64) - vecs[2].to(_F64)) * vecs[3].to(_F64)
    m1, m2 = S[0] / npix, S[1] / npix
    dy = sc * (r.da - m1 - xhat * m2)
    e = 8 * U * sc.abs() * (r.da.abs() + m1.abs() + xhat.abs() * m2.abs()) + sc.abs() * r.e_da
    if old is not None:
        dy = dy + old.to(_F64)
        e = e + U * dy.abs()
    return stored(dy, e, dtype)
