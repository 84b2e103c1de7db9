"""The case matrix of csrc/elementwise.hip shared by tests/test_elementwise_reference.py (CPU: the fp64 reference of
oracle/elementwise.py and its bounds) and tests/test_gpu_elementwise_elements.py (GPU: the kernels held to them), with the launch rules
restated, the inputs and the sentinel-framed buffers (those of tests/stem_cases.py).

Launch rules of the library, restated here so that every case can assert the path it is named for:
  EPV                 elements per 16-byte vector: 4 in f32, 8 in bf16 / f16.  CV = C / EPV.
  ew_grid(v)          clamp(ceil(v / 256), 1, 4096) workgroups of 256 threads, one vector per thread and trip: the grid-stride loop turns
                      beyond 4096 * 256 = 1048576 vectors.  dot: clamp(ceil(v / 2048), 1, 1024): it turns beyond 1024 * 256 vectors and
                      every thread makes 8 trips from 1024 * 2048 on.
  maxpool_tile_ok     stride <= 1, k odd, H * W <= 1024, C % 4 == 0: the LDS-plane kernels, one workgroup of min(1024, 64 ceil(HW / 64))
                      threads per (image, channel vector), xcd_remap over B * CV workgroups (remainder branch when B * CV % 8 != 0);
                      forward 40 HW bytes of LDS, backward 64 HW (65536 at 32 x 32).  Everything else: the generic kernels through
                      ew_grid(B * H * W * CV).
  the K switch        k in {2, 3, 5, 9, 13}: the <T, k> instantiation; any other k <= 15: <T, 0> (runtime k).
  se_pool             CVB = smallest power of two >= CV, at most 16; PY = 256 / CVB pixel lanes; gx = ceil(CV / CVB); with a scratch
                      HS doubles from 1 while HS < 16, gx * B * HS < 1024 and HW / (2 HS) >= 8 PY; chunk = ceil(HW / HS).
  se_rows_grid(R, B)  gx = ceil(R / 16); gy = clamp(512 / gx, 1, B); bper = ceil(B / gy) images per workgroup, ceil(B / bper) slices.
                      dyk_se_fc_fwd calls it with (Cs, B) for h and with (C, B) for scale.
  se_scale            CVB = smallest power of two >= CV, at most 32; PY = 256 / CVB; gx = ceil(CV / CVB); gy = clamp(ceil(HW / (8 PY)),
                      1, max(1, 4096 / (gx B))); with the reduce nz = clamp(768 / (gx gy), 1, B) workgroups along the images (the image
                      loop turns when nz < B), without it nz = B.
  head                permute: ew_grid over elements; bias gradient: one 1024-thread workgroup per channel, four loads per trip while
                      r + 3072 < cells, then single loads.
"""
import collections
import functools
import itertools

import torch

from oracle import elementwise as O
from stem_cases import SENTINEL, Buf, Flat  # noqa: F401  (the sentinel-framed buffers: one definition for both suites)

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
EW_CAP = 4096 * 256


def epv(dt):
    return 4 if dt == "f32" else 8


def ew_grid(vecs):
    return max(1, min(4096, -(-vecs // 256)))


def dot_grid(vecs):
    return max(1, min(1024, -(-vecs // 2048)))


def dot_trips(vecs):
    return -(-vecs // (dot_grid(vecs) * 256))


# row layouts of a channels-last tensor of C channels: (ld, channel offset).  `slice`: how a producer writes into a concat buffer
def layout(C, name):
    return {"tight": (C, 0), "slice": (C + 24, 8)}[name]


def nhwc(x, dt, lay="tight", fill=True):
    """an armed Buf holding the NCHW tensor x (or only shaped like it) in the given row layout"""
    B, C, H, W = x.shape
    ld, off = layout(C, lay)
    b = Buf(B, H, W, C, DTYPES[dt], ld=ld, off=off)
    if fill:
        b.put(x)
    return b.arm()


# ---------------------------------------------------------------------------------------------------- max pool
def tile_ok(k, stride, H, W, C):
    return stride <= 1 and k % 2 == 1 and H * W <= 1024 and C % 4 == 0


def pool_K(k):
    return k if k in (2, 3, 5, 9, 13) else 0


def tile_threads(HW):
    return min(1024, -(-HW // 64) * 64)


TILE_MAPS = [(1, 1), (2, 3), (7, 9), (16, 20), (1, 1024), (32, 32)]
TILE_KS = [1, 3, 5, 7, 9, 13, 15]
TILE_C = {"bf16": [8, 24, 40], "f32": [4, 12], "f16": [8, 24, 40]}
GENERIC_MAP = (33, 32)
GENERIC_KS = [3, 5, 9, 13, 7, 15]
STRIDED = [(2, 2), (3, 2), (5, 2), (9, 2), (13, 2), (4, 1), (2, 1), (3, 3), (15, 8)]
STRIDED_MAPS = [(7, 9), (3, 5), (1, 1)]
BIG_POOL = (1025, 1024)            # B = 1, C = 8, bf16, k = 3: 1049600 vectors > 1048576


def tile_matrix():
    """(H, W, k): every map with every window; tile_variants() gives the channels, types and layouts of each"""
    return [(H, W, k) for (H, W) in TILE_MAPS for k in TILE_KS]


def tile_variants(H, W, k):
    """[(dtype, C, B, layout)] of one (map, window): every C of every type.  `layout` is where the forward reads and the store-form
    backward reads; every launch writes the OTHER layout, and the argmax-less forward and the accumulate-form backward swap the two, so
    each variant runs both on both sides; the starting layout alternates with the case.  B * CV is never a multiple of 8 (3, 9, 15 or
    2, 6, 10: the remainder branch of xcd_remap)"""
    i = TILE_MAPS.index((H, W)) + TILE_KS.index(k)
    B = 2 if H * W >= 1024 else 3
    out = [(dt, C, B, ("tight", "slice")[(i + j) % 2]) for dt in ("bf16", "f32", "f16") for j, C in enumerate(TILE_C[dt])]
    for dt, C, B_, lay in out:
        assert tile_ok(k, 1, H, W, C) and (B_ * (C // epv(dt))) % 8 != 0
    return out


def pool_shape(H, W, k, stride):
    return O.pool_out(H, k, stride), O.pool_out(W, k, stride)


def _seed(*v):
    return 7000 + sum((i + 3) * 131 * int(x) for i, x in enumerate(v))


@functools.lru_cache(maxsize=None)
def pool_input(B, C, H, W):
    """half-integer-quantised normals (ties in every window; all representable in bf16 and fp16) with, where the tensor has room:
    a plane of -0.0 / +0.0 / -1 (image B - 1, channel 2), zeros signed by pixel parity everywhere, a single NaN (image 0, channel 0),
    NaNs at the first and the last pixel and two neighbours (channel 1: several in one window, at its first and last tap), +inf
    (channel 2) and a plane of -inf (channel 3).  Large tensors (the grid-stride case) keep ties, signed zeros, one NaN, one +inf"""
    g = torch.Generator().manual_seed(_seed(B, C, H, W))
    x = (torch.randn(B, C, H, W, generator=g) * 3.0).round() / 2.0
    par = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2 == 0)
    if C > 2 and H * W <= 4096:
        pl = torch.randint(0, 3, (H, W), generator=g).float()
        x[B - 1, 2] = torch.where(pl == 2, torch.full_like(pl, -1.0), torch.zeros_like(pl))
    x = torch.where((x == 0) & par, torch.full_like(x, -0.0), x)
    x[0, 0, H // 2, W // 2] = float("nan")
    if C > 2:
        x[0, 2, H // 3, W // 3] = float("inf")
    if H * W <= 4096:
        for (yy, xx) in ((0, 0), (H - 1, W - 1), (0, min(1, W - 1)), (min(1, H - 1), 0)):
            x[0, 1, yy, xx] = float("nan")
        if C > 3:
            x[0, 3] = float("-inf")
    return x


@functools.lru_cache(maxsize=None)
def pool_ref(B, C, H, W, k, stride):
    """(values float32 NCHW, codes uint8 NCHW) of the oracle; values of pool_input are exact in every storage type"""
    v, c = O.pool_fwd(pool_input(B, C, H, W), k, stride)
    return v.float(), c


@functools.lru_cache(maxsize=None)
def pool_grad(B, C, Ho, Wo, dt, nan):
    """the output gradient rounded to storage (float32 NCHW); nan: NaN at a few outputs"""
    g = torch.Generator().manual_seed(_seed(B, C, Ho, Wo, 5))
    dy = O.store(torch.randn(B, C, Ho, Wo, generator=g), DTYPES[dt]).float()
    if nan:
        dy[0, 0, 0, 0] = float("nan")
        dy[B - 1, C - 1, Ho - 1, Wo - 1] = float("nan")
        dy[0, 1, Ho // 2, Wo // 2] = float("nan")
    return dy


@functools.lru_cache(maxsize=None)
def pool_bwd_ref(B, C, H, W, k, stride, dt, nan, accumulate):
    """(gradient, old or None, target, bound) of one backward problem, gathered with the oracle's codes"""
    code = pool_ref(B, C, H, W, k, stride)[1]
    dy = pool_grad(B, C, code.shape[2], code.shape[3], dt, nan)
    old = rand_tensor(B, C, H, W, dt, 9) if accumulate else None
    return (dy, old) + O.pool_bwd(dy, code, k, stride, H, W, DTYPES[dt], old)


@functools.lru_cache(maxsize=None)
def rand_tensor(B, C, H, W, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(_seed(B, C, H, W, seed))
    return O.store(scale * torch.randn(B, C, H, W, generator=g), DTYPES[dt]).float()


# ---------------------------------------------------------------------------------------------------- upsample / axpby / dot
UP_MAPS = [(1, 1), (7, 9)]
UP_C = [8, 24]
BIG_UP_FWD = (513, 512)            # input map; 4 * 513 * 512 output vectors at C = 8 bf16 = 1050624 > 1048576
BIG_UP_BWD = (1025, 1024)          # input-gradient map: 1049600 vectors
BIG_AXPBY = (1025, 1024)
BIG_DOT = (1025, 2048)             # 2099200 vectors > 1024 * 2048: nine trips for some threads

# b present, p0 present, p1 present, accumulate, in place (out == a)
AXPBY_FORMS = [f for f in itertools.product((False, True), repeat=5) if not (f[2] and not f[0])]
AXPBY_LDS = [("tight", "tight", "tight"), ("slice", "tight", "slice"), ("tight", "slice", "slice")]     # (a, b, out) row layouts


WFUSE_N = [1, 2, 3, 5, 64]


@functools.lru_cache(maxsize=None)
def wfuse_problem(n):
    """(w in [-12, 12] with both ends and 0 among them, red fp64, the dw the launch adds to)"""
    g = torch.Generator().manual_seed(_seed(n, 77))
    w = (torch.rand(n, generator=g) * 2 - 1) * O.WFUSE_RANGE
    w[0] = -O.WFUSE_RANGE
    if n > 2:
        w[1], w[2] = O.WFUSE_RANGE, 0.0
    return w, torch.randn(n, generator=g, dtype=torch.float64) * 100.0, torch.randn(n, generator=g)


# ---------------------------------------------------------------------------------------------------- squeeze-excitation
def se_pool_geo(C, dt, B, HW, scratch):
    """(CVB, PY, gx, HS, chunk)"""
    CV = C // epv(dt)
    CVB = 1
    while CVB < CV and CVB < 16:
        CVB *= 2
    PY, gx, HS = 256 // CVB, -(-CV // CVB), 1
    if scratch:
        while HS < 16 and gx * B * HS < 1024 and HW // (HS * 2) >= PY * 8:
            HS *= 2
    return CVB, PY, gx, HS, -(-HW // HS)


def se_pool_m(C, dt, B, HW, scratch):
    CVB, PY, gx, HS, chunk = se_pool_geo(C, dt, B, HW, scratch)
    return -(-chunk // PY) + PY + HS + 1


SE_POOL_C = [("bf16", 8), ("bf16", 24), ("bf16", 136), ("f32", 4)]
SE_POOL_MAPS = [(1, 1), (1, 5), (16, 17), (43, 49), (64, 64)]
# what the named cases must reach: (dtype, C, map, scratch) -> (CVB, HS)
SE_POOL_PATHS = {
    ("bf16", 8, (1, 1), True): (1, 1), ("bf16", 24, (1, 5), True): (4, 1), ("bf16", 136, (16, 17), True): (16, 2),
    ("bf16", 136, (43, 49), True): (16, 16), ("bf16", 8, (64, 64), True): (1, 2), ("bf16", 136, (43, 49), False): (16, 1),
}


def se_rows_grid(R, B):
    """(gx, slices, bper)"""
    gx = -(-R // 16)
    gy = max(1, min(B, 512 // gx))
    bper = -(-B // gy)
    return gx, -(-B // bper), bper


SE_FC = [(8, 4, 1), (64, 16, 3), (260, 132, 5), (960, 240, 16), (960, 240, 17), (8192, 8, 1), (64, 16, 256)]
SE_FC_BPER = {(960, 240, 16): 2, (960, 240, 17): 3}          # bper of the scale launch (R = C)

SeProblem = collections.namedtuple("SeProblem", "C Cs B pooled w1 b1 w2 b2 dscale h dt1 t2 old")


@functools.lru_cache(maxsize=None)
def se_problem(C, Cs, B):
    """parameters, pooled, dscale and a workspace h | dt1 | t2 the TEST writes for the backward launches: t2 holds exact +-3 (derivative
    0: the inequality is strict) and values either side, h exact zeros (derivative 0) among positive and negative values"""
    g = torch.Generator().manual_seed(_seed(C, Cs, B))
    r = lambda *s: torch.randn(*s, generator=g)
    pooled, dscale = r(B, C), r(B, C)
    w1, b1, w2, b2 = r(Cs, C) * (2.0 / C ** 0.5), r(Cs) * 0.1, r(C, Cs) * (2.0 / Cs ** 0.5), r(C) * 0.5
    h = r(B, Cs).clamp(min=0.0)
    h[:, ::3] = 0.0
    h[:, 1::7] = -0.5                                  # (never stored by the forward; the rule is h > 0)
    dt1 = r(B, Cs)
    t2 = r(B, C) * 3.0
    t2[:, ::5] = 3.0
    t2[:, 1::5] = -3.0
    t2[:, 2::11] = 2.9999998
    old = {"dw1": r(Cs, C) * 0.5, "db1": r(Cs) * 0.5, "dw2": r(C, Cs) * 0.5, "db2": r(C) * 0.5}
    return SeProblem(C, Cs, B, pooled, w1, b1, w2, b2, dscale, h, dt1, t2, old)


def se_scale_geo(C, dt, B, HW, reduce):
    """(CVB, PY, gx, gy, nz)"""
    CV = C // epv(dt)
    CVB = 1
    while CVB < CV and CVB < 32:
        CVB *= 2
    PY, gx = 256 // CVB, -(-CV // CVB)
    gy = max(1, min(-(-HW // (PY * 8)), max(1, 4096 // (gx * B))))
    nz = max(1, min(B, 768 // (gx * gy))) if reduce else B
    return CVB, PY, gx, gy, nz


def se_reduce_m(C, dt, B, HW):
    """roundings on the longest path of one channel's sum: images per workgroup x pixels per lane, the PY lane sums, the products"""
    CVB, PY, gx, gy, nz = se_scale_geo(C, dt, B, HW, True)
    return -(-B // nz) * -(-HW // (gy * PY)) + PY + 2


@functools.lru_cache(maxsize=None)
def se_reduce_problem(B, C, H, W, dt):
    """(dz, yraw, old, p0, p1, vecs [4, C]) distributed like the inputs of test_se_scale_backward_carries_the_batchnorm_backward_reduce"""
    g = torch.Generator().manual_seed(_seed(B, C, H, W, 61))
    dz, old = rand_tensor(B, C, H, W, dt, 62), rand_tensor(B, C, H, W, dt, 63)
    yraw = rand_tensor(B, C, H, W, dt, 64, 2.0)
    p0, p1 = torch.rand(B, C, generator=g), torch.randn(B, C, generator=g)
    vecs = torch.stack([1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
                        1.0 + 0.1 * torch.rand(C, generator=g)])
    return dz, yraw, old, p0, p1, vecs


SE_SCALE_C = [("bf16", 8), ("bf16", 72), ("bf16", 264), ("f32", 4)]
SE_SCALE_MAPS = [(1, 1), (3, 5), (33, 17)]
SE_SCALE_LOOP = (32, 264, 25, 32)                     # with the reduce: nz = 29 < B

# ---------------------------------------------------------------------------------------------------- head
HEAD_MAPS = [(5, 7), (1, 3073), (64, 80), (1, 4097)]       # cells 35 (tail loop only), 3073 (one four-load trip, lane 0), 5120, 4097 (main + tail)
HEAD_NA, HEAD_NO = 3, 6
HEAD_LD = {"f32": [18, 24, 32], "bf16": [24, 32]}


def head_main_trips(cells):
    """lanes that take the four-load trip at least once"""
    return max(0, min(1024, cells - 3072))
