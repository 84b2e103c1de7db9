"""The case matrix of csrc/bn_act.hip shared by tests/test_bn_act_reference.py (CPU: the fp64 reference of oracle/bn_act.py and its
bounds) and tests/test_gpu_bn_act_elements.py (GPU: the kernels held to them): shapes with the launch geometry each must reach, seeded
problems, statistics replicas, the kink field and the sentinel-framed row buffers (those of tests/stem_cases.py).

Tensors are rows [P, C]: P pixels of C channels, what the kernels see of a channels-last tensor.  Geometry (oracle/bn_act.py ew_grid):
CV = C / EPV vectors in groups of CVB = the power of two >= CV, at most 32; PY = 256 / CVB pixel lanes; gx = ceil(CV / CVB);
gy = clamp(ceil(P / 8 PY), 1, 2048 / gx) workgroups, each a contiguous chunk of ceil(ceil(P / gy) / PY) PY pixels walked four rows per trip.
"""
import collections
import functools

import torch

from elementwise_cases import DTYPES  # noqa: F401  (one definition of the storage types; the slice rows here are C + 3 EPV wide: row_layout)
from oracle import bn_act as O
from stem_cases import SENTINEL, Buf, Flat  # noqa: F401

Shape = collections.namedtuple("Shape", "id npix C")
# the smallest shapes that turn each branch; GEOMETRY is what each must reach, asserted by the tests from oracle/bn_act.py's restatement
SHAPES = [
    Shape("1", 1, {"bf16": 8, "f16": 8, "f32": 4}),            # one live thread; count == 1
    Shape("35", 35, {"bf16": 24, "f16": 24, "f32": 12}),       # CV = 3 < CVB = 4: an idle column; npix < PY
    Shape("2049", 2049, {"bf16": 8}),                          # gy = 2, five rows per thread: the second trip is partial
    Shape("4099", 4099, {"bf16": 72}),                         # CVB = 16, gy = 33 > 16 replicas, the last chunk has 3 pixels
    Shape("577", 577, {"bf16": 264, "f16": 264, "f32": 132}),  # gx = 2 with a tail group of ONE vector, gy = 10, the last chunk has 1 pixel
    Shape("63", 63, {"bf16": 264}),                            # gx = 2, gy = 1, eight rows per thread
]
BIG = Shape("65537", 65537, {"bf16": 264, "f32": 132})         # gy capped at 1024, nine rows per thread, 113 empty workgroups
BY_ID = {s.id: s for s in SHAPES + [BIG]}
#            id       CVB  PY  gx    gy  chunk rows empty last
GEOMETRY = {"1": (1, 256, 1, 1, 256, 1, 0, 1), "35": (4, 64, 1, 1, 64, 1, 0, 35), "2049": (1, 256, 1, 2, 1280, 5, 0, 769),
            "4099": (16, 16, 1, 33, 128, 8, 0, 3), "577": (32, 8, 2, 10, 64, 8, 0, 1), "63": (32, 8, 2, 1, 64, 8, 0, 63),
            "65537": (32, 8, 2, 1024, 72, 9, 113, 17)}
SMALL = [(s.id, dt) for s in SHAPES for dt in s.C]
TRAIN = [(sid, dt) for sid, dt in SMALL if dt != "f16"]         # the backward kernels and the fused forward: bf16 | f32

ACTS = O.ACTS
FIN_SLOTS = [1, 4, 32, 33, 256]
FUSED_SLOTS = [1, 3, 4, 7, 16, 23, 32]
APPLY_SLOTS = [1, 7, 8, 16, 25, 31]
REDUCE_SLOTS = [1, 4, 16]
ROUTE_PAD, ROUTE_OFF = 40, 24                                   # a [route]'s joint reduction: Ctot = C + 40, this layer's columns from 24 on
LAYOUTS = ["tight", "slice"]
EPS, MOMENTUM = 1e-5, 0.1


def geometry(sid, dt, reduce=False):
    s = BY_ID[sid]
    return (O.reduce_grid if reduce else O.ew_grid)(s.C[dt], s.npix, dt)


def assert_geometry(sid, dt):
    for red in (False, True):
        g = geometry(sid, dt, red)
        assert (g.CVB, g.PY, g.gx, g.gy, g.chunk, g.rows, g.empty, g.last) == GEOMETRY[sid], (sid, dt, g)
    return g


def row_layout(C, dt, name):
    """(ld, channel offset): tight rows, or the slice [EPV : EPV + C] of rows of C + 3 EPV elements (chan_slice of a joint raw tensor)"""
    e = O.epv(dt)
    return {"tight": (C, 0), "slice": (C + 3 * e, e)}[name]


def rows_buf(P, C, dt, lay, src=None):
    """an armed Buf of P rows of C channels in the given layout, sentinel-filled or holding src [P, C]"""
    ld, off = row_layout(C, dt, lay)
    b = Buf(1, 1, P, C, DTYPES[dt], ld=ld, off=off)
    if src is not None:
        b.t.copy_(src.view(1, 1, P, C).to(DTYPES[dt]))
    return b.arm()


def get_rows(b):
    return b.t.cpu().reshape(-1, b.t.shape[3]).double()


def _seed(*v):
    return 9000 + sum((i + 5) * 173 * int(x) for i, x in enumerate(v))


def _rows(P, C, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(_seed(P, C, seed))
    return O.store(scale * torch.randn(P, C, generator=g) + shift, DTYPES[dt]).float()


Problem = collections.namedtuple("Problem", "sid dt P C y g res old vecs")


@functools.lru_cache(maxsize=None)
def problem(sid, dt):
    """y ~ N(0.5, 2), gradient, residual and old ~ N(0, 1), all rounded to storage; vecs = scale | shift | mean | rstd [4, C] fp32, drawn
    independently (the kernels take four vectors): scale of either sign in +-[0.5, 1.5], so that t = y scale + shift passes -3, 0, 3 and 6"""
    s = BY_ID[sid]
    P, C = s.npix, s.C[dt]
    g = torch.Generator().manual_seed(_seed(P, C, 1))
    sign = torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    vecs = torch.stack([sign * (0.5 + torch.rand(C, generator=g)), 0.5 * torch.randn(C, generator=g), 0.5 + 0.1 * torch.randn(C, generator=g),
                        0.4 + 0.2 * torch.rand(C, generator=g)]).float().contiguous()
    return Problem(sid, dt, P, C, _rows(P, C, dt, 2, 2.0, 0.5), _rows(P, C, dt, 3), _rows(P, C, dt, 4), _rows(P, C, dt, 5), vecs)


@functools.lru_cache(maxsize=None)
def replicas(C, slots, npix, seed=0):
    """[slots, 2, C] fp64: reduction sums of mixed signs and magnitudes (a dropped or doubled replica moves S / N by far more than a bound)"""
    g = torch.Generator().manual_seed(_seed(C, slots, seed, 7))
    mag = torch.tensor([0.02, 0.3, 1.0, 4.0], dtype=torch.float64)[torch.randint(0, 4, (slots, 1, 1), generator=g)]
    r = torch.randn(slots, 2, C, generator=g, dtype=torch.float64)
    r = torch.where(r.abs() < 0.2, r.sign() * 0.2, r)
    return (r * mag * 0.2 * npix).contiguous()


def route_red(red):
    """the replicas as columns of a wider reduction: ([slots, 2 Ctot] with the sentinel everywhere else, H, W, column offset)"""
    slots, _, C = red.shape
    ctot = C + ROUTE_PAD
    wide = torch.full((slots, 2 * ctot), SENTINEL, dtype=torch.float64)
    wide[:, ROUTE_OFF:ROUTE_OFF + C] = red[:, 0]
    wide[:, ctot + ROUTE_OFF:ctot + ROUTE_OFF + C] = red[:, 1]
    return wide, 2 * ctot, ctot, ROUTE_OFF


# ---------------------------------------------------------------------------------------------------- finalize
FinProblem = collections.namedtuple("FinProblem", "C count slots stats gamma beta rm rv const zero_gamma")
_MEANS = [0.5, -3.0, 100.0, 1e-3, 0.0, -40.0, 7.0, 0.25]
_VARS = [4.0, 1e-4, 1.0, 0.25, 2.0, 3e-5, 9.0, 0.5, 1e-2]


def pixel_split(count, slots):
    """whole pixels per replica: [slots] fp64 summing to count"""
    base, rem = divmod(count, slots)
    k = torch.full((slots,), float(base), dtype=torch.float64)
    k[:rem] += 1
    return k


def const_stats(count, slots, base=1.0, below=0.0):
    """(v, s1 [slots], s2 [slots]) of a channel every pixel of which is the fp32 value v: replica r holds fp32(k_r v) and
    fp32(k_r v^2) for k_r whole pixels, as a producer's fp32 partial sums leave them; v is the first of a ladder for which the fp64
    S2 / n - (S1 / n)^2 of the exactly summed replicas is NEGATIVE (below `below`).  base 2^22: the rounding of the difference exceeds eps, so an unclamped variance + eps is negative too"""
    k, n = pixel_split(count, slots), float(count)
    for i in range(1, 2000):
        v = float(torch.tensor(base * (1.1 + 0.003 * i), dtype=torch.float32))
        s1, s2 = (k * v).float().double(), (k * (v * v)).float().double()
        S1, S2 = O.exact_sum(s1.view(-1, 1))[0], O.exact_sum(s2.view(-1, 1))[0]
        if float(S2 / n - (S1 / n) ** 2) < below:
            return v, s1, s2
    raise AssertionError("no constant with a negative fp64 variance at count %d, %d replicas" % (count, slots))


HUGE = 2.0 ** 22


@functools.lru_cache(maxsize=None)
def fin_problem(C, count, slots, seed=0):
    """statistics replicas of channels whose mean / variance walk _MEANS x _VARS (|mean| up to 100 sigma, variances down to eps), spread
    over the replicas with weights of mixed sign and magnitude that sum to one.  Channel 1 is CONSTANT (const_stats: the fp64 variance
    is negative before the clamp), channel 3 constant at 2^22, channel 2 has gamma == 0.  count == 1: s2 = s1^2 in
    every channel"""
    g = torch.Generator().manual_seed(_seed(C, count, slots, seed, 3))
    n = float(count)
    mean = torch.tensor([_MEANS[c % len(_MEANS)] for c in range(C)], dtype=torch.float64) * (1 + 0.1 * torch.rand(C, generator=g, dtype=torch.float64))
    var = torch.tensor([_VARS[c % len(_VARS)] for c in range(C)], dtype=torch.float64) * (1 + 0.1 * torch.rand(C, generator=g, dtype=torch.float64))
    if count == 1:
        var = torch.zeros(C, dtype=torch.float64)
    w = torch.randn(slots, 1, generator=g, dtype=torch.float64) * torch.tensor([0.1, 1.0, 3.0], dtype=torch.float64)[torch.randint(0, 3, (slots, 1), generator=g)]
    w[0] += 1.0 - w.sum()
    stats = torch.empty(slots, 2, C, dtype=torch.float64)
    stats[:, 0] = w * (n * mean)
    stats[:, 1] = w * (n * (var + mean * mean))
    const = None
    if count >= 35 and C > 2:
        const = 1
        _, stats[:, 0, 1], stats[:, 1, 1] = const_stats(count, slots)
        if C > 3:                                   # channel 3: the same at 2^22, where the negative difference is below -eps
            _, stats[:, 0, 3], stats[:, 1, 3] = const_stats(count, slots, HUGE, -2 * EPS)
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::5] *= -1.0
    zero_gamma = None
    if C > 2:
        gamma[2], zero_gamma = 0.0, 2
    beta = torch.randn(C, generator=g)
    beta[::3] = (mean * gamma.double() / (var + EPS).sqrt()).float()[::3]          # shift cancels: |shift| << |mean scale|
    return FinProblem(C, count, slots, stats.contiguous(), gamma, beta, 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g),
                      const, zero_gamma)


def fin_ref(p, gamma=True, beta=True, running=True):
    return O.finalize(p.stats, p.count, EPS, p.gamma if gamma else None, p.beta if beta else None, MOMENTUM,
                      p.rm if running else None, p.rv if running else None)


@functools.lru_cache(maxsize=None)
def fold_problem(C, seed=0):
    """(gamma, beta, running_mean, running_var): variances from 1e-6 (below eps) to 50"""
    g = torch.Generator().manual_seed(_seed(C, seed, 11))
    rv = torch.exp(torch.rand(C, generator=g) * 17.0 - 13.0)
    rv[0] = 0.0
    return 0.5 - torch.rand(C, generator=g) * 2, torch.randn(C, generator=g), 3.0 * torch.randn(C, generator=g), rv


# ---------------------------------------------------------------------------------------------------- the kink field
def _nb(v):
    """the two bf16 neighbours of a bf16 value"""
    b = torch.tensor([v], dtype=torch.bfloat16).view(torch.int16)
    return [float((b + d).view(torch.bfloat16)) for d in (1, -1)]


MIN_NORMAL = 2.0 ** -126
KINK_VALUES = [0.0, -0.0, MIN_NORMAL, -MIN_NORMAL, 3.0] + _nb(3.0) + [-3.0] + _nb(-3.0) + [6.0] + _nb(6.0) + [1.0, -1.0, 20.0]
# the project's convention, which is torch's: the derivative AT the kink
KINK_CONVENTION = {"leaky": {0.0: 0.1}, "relu": {0.0: 0.0}, "relu6": {0.0: 0.0, 6.0: 0.0}, "hard-sigmoid": {3.0: 0.0, -3.0: 0.0},
                   "hard-swish": {-3.0: -0.5, 3.0: 1.5}}


def kink_field():
    """y [1, 16]: one pixel, one value per channel; scale 1, shift 0 (t == y exactly), mean 0, rstd 1 (xhat == y), gradient 1"""
    assert len(KINK_VALUES) == 16
    y = torch.tensor(KINK_VALUES, dtype=torch.float32).view(1, 16)
    assert torch.equal(y.bfloat16().float(), y)
    vecs = torch.stack([torch.ones(16), torch.zeros(16), torch.zeros(16), torch.ones(16)]).contiguous()
    return y, torch.ones(1, 16), vecs


def kink_da(act):
    """the derivative the kernels must produce on the kink field, as fp32: the fp32 constants 0.1f and 1 / 6f, hard-swish's
    fp32(fp32(y * fp32(1 / 3)) + 0.5) (exact or a single rounding at every value of the field)"""
    y = kink_field()[0]
    if act == "hard-swish":
        mid = (y * torch.tensor(1.0 / 3.0)) + 0.5
        return torch.where(y < -3, torch.zeros_like(y), torch.where(y <= 3, mid, torch.ones_like(y)))
    return O._ACT_D[act][0](y.double()).float()
