"""The stem-convolution case matrix shared by tests/test_stem_reference.py (CPU: the fp64 reference of oracle/stem.py and its
bounds) and tests/test_gpu_stem_elements.py (GPU: csrc/stem.hip held to them), with the inputs, the cached references and the
sentinel-framed buffers.

Geometry of the kernels: a SEGMENT is 128 output pixels of one output row (STEM_SEG).  The MFMA forward (stem_fwd_u8t_kernel:
uint8 image, 32 filters, bf16 | f16, W % 4 == 0, 4-byte-aligned image) walks a segment in tiles of 32 pixels and gives a one-wave
workgroup ceil(nsegs / 3072) segments; the uint8 weight gradient (stem_wgrad_u8_kernel: bf16, lddy == Cout, W % 4 == 0, 4-byte-aligned
image, 16-byte-aligned gradient) takes 16 pixels per trip, the generic one (stem_wgrad_kernel) 8; both give a workgroup
ceil(nsegs / 4096) segments and write one partial plane per workgroup, which stem_wgrad_fold_kernel folds 512 planes per trip.
The scalar forward (stem_fwd_kernel) caps its grid at 2048 workgroups of 256 pixels.
"""
import collections
import functools

import torch

from oracle import stem as O

SEG = 128
Geo = collections.namedtuple("Geo", "id B H W")

GEOS = [
    Geo("4x4", 2, 4, 4),            # smallest word-load width; Wo 4 / 2; one masked tile
    Geo("5x12", 3, 5, 12),          # odd H: bottom halo at stride 2
    Geo("9x47", 2, 9, 47),          # W % 4 != 0: uint8 through the scalar forward and the byte-load weight gradient
    Geo("3x128", 2, 3, 128),        # stride 1: exactly one full segment, the right-halo word wholly outside the image
    Geo("5x132", 2, 5, 132),        # stride 1: a full segment + a 4-pixel segment (first store half masked, second dead)
    Geo("6x300", 1, 6, 300),        # stride 1: 2 full + 44 (full tile + 12-pixel tile).  Stride 2: 1 full + 22 (second store half partly masked)
    Geo("6x256", 1, 6, 256),        # stride 2: Wo = 128 exactly; even H (no bottom halo)
    Geo("7x520", 1, 7, 520),        # stride 2: Wo = 260, pixels 126 / 127 of full segments read the second staged word.  Stride 1: 4 full + 8
]
# the three large cases: no smaller shape puts two segments into one workgroup or makes the loops turn
BIG_FWD = Geo("205x260x5", 5, 205, 260)       # forward, uint8, 32 filters, stride 1, bf16, statistics: nsegs 3075 > 3072, two segments per
#                                               workgroup at three per row: workgroups straddle rows and images
BIG_WGRAD = Geo("205x260x7", 7, 205, 260)     # weight gradient, exact field, stride 1: nsegs 4305 > 4096, two segments per workgroup, 2153
#                                               planes (fold loop: five trips)
BIG_SCALAR = Geo("1025x512", 1, 1025, 512)    # scalar forward, 16 filters, bf16, float image, stride 1: 524800 pixels > 2048 * 256 (grid-stride loop)
BY_ID = {g.id: g for g in GEOS + [BIG_FWD, BIG_WGRAD, BIG_SCALAR]}

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}
ACTS = O.ACTS                                   # linear, leaky, relu6, hard-swish, mish
F16_OVERFLOW_SCALE = 6.0e4                      # y * scale passes 65504 for |y| > 1.1


def img_kind(u8):
    return "u8" if u8 else "float"


def forward_matrix():
    """(geometry, filters, stride, uint8 image?, storage type): every small geometry in every combination"""
    return [(g.id, co, s, u8, dt) for g in GEOS for co in (16, 32) for s in (1, 2) for u8 in (True, False) for dt in ("bf16", "f32", "f16")]


# dy layouts: (lddy, channel offset of the slice).  `wide32`: 16 filters in 32-channel rows; `slice`: [8 : 8 + Cout] of ld = Cout + 24 -- the
# generic lddy branch of stem_wgrad_kernel (neither 16 nor 32)
def dy_layouts(cout):
    return ["tight", "slice"] + (["wide32"] if cout == 16 else [])


def dy_layout(cout, name):
    return {"tight": (cout, 0), "wide32": (32, 0), "slice": (cout + 24, 8)}[name]


def wgrad_matrix():
    return [(g.id, co, s, u8, dt, lay) for g in GEOS for co in (16, 32) for s in (1, 2) for u8 in (True, False) for dt in ("bf16", "f32")
            for lay in dy_layouts(co)]


def out_hw(geo, stride):
    return O.out_hw(geo.H, geo.W, stride)


def mfma_forward(geo, cout, u8, dt, aligned=True):
    """the dispatch condition of stem_fwd_u8t_kernel, restated"""
    return u8 and cout == 32 and dt in ("bf16", "f16") and geo.W % 4 == 0 and aligned


def u8_wgrad(geo, cout, u8, dt, lddy, aligned=True):
    """the dispatch condition of stem_wgrad_u8_kernel (sum, then one 1/255), restated"""
    return u8 and dt == "bf16" and lddy == cout and geo.W % 4 == 0 and aligned


def segments(geo, stride):
    Ho, Wo = out_hw(geo, stride)
    spr = -(-Wo // SEG)
    return spr, geo.B * Ho * spr


def forward_segs_per_wg(geo, stride):
    nsegs = segments(geo, stride)[1]
    return -(-nsegs // min(nsegs, 3072))


def wgrad_planes(geo, stride):
    """(segments per workgroup, planes) of the weight-gradient launch: at most 4096 one-wave workgroups"""
    nsegs = segments(geo, stride)[1]
    spw = max(1, -(-nsegs // 4096))
    return spw, -(-nsegs // spw)


def seg_index(geo, stride):
    """[B, Ho, Wo] int64: the segment an output pixel belongs to"""
    Ho, Wo = out_hw(geo, stride)
    spr = segments(geo, stride)[0]
    rows = torch.arange(geo.B * Ho).view(geo.B, Ho, 1)
    return rows * spr + (torch.arange(Wo) // SEG).view(1, 1, Wo)


def _seed(geo, *extra):
    return 4000 + 97 * list(BY_ID).index(geo.id) + sum((i + 1) * int(e) for i, e in enumerate(extra))


# ---------------------------------------------------------------------------------------------------- forward
FwdProblem = collections.namedtuple("FwdProblem", "geo cout stride img8 imgf w scale shift ref")


@functools.lru_cache(maxsize=None)
def fwd_problem(geo_id, cout, stride):
    """uint8 image and its float twin (img8.float() / 255: one reference serves both kinds), asymmetric random weights [Cout, 27], the
    eval epilogue's scale / shift (y * scale + shift spans both signs and exceeds 6) and the fp64 reference; computed once, shared,
    never modified"""
    geo = BY_ID[geo_id]
    g = torch.Generator().manual_seed(_seed(geo, cout, stride))
    img8 = torch.randint(0, 256, (geo.B, 3, geo.H, geo.W), dtype=torch.uint8, generator=g)
    imgf = (img8.float() / 255.0).contiguous()
    w = (torch.randn(cout, 27, generator=g) * 0.3).contiguous()
    scale = 2.5 + torch.rand(cout, generator=g)
    shift = 1.25 + 0.5 * torch.rand(cout, generator=g)
    return FwdProblem(geo, cout, stride, img8, imgf, w, scale, shift, O.reference(img8, w, stride))


CONST_GEO = Geo("const", 2, 17, 24)


@functools.lru_cache(maxsize=None)
def const_problem(cout, stride):
    """the constant field of dwconv_cases.const_problem transposed to the stem: every pixel 255 (x = 1), every weight (1 + 2^-10) / 27.
    Interior accumulators are ~ 1 + 2^-10 and store as 1.0 in bf16: statistics taken from the STORED values are off by ~ 1e-3 relative"""
    geo = CONST_GEO
    img8 = torch.full((geo.B, 3, geo.H, geo.W), 255, dtype=torch.uint8)
    w = torch.full((cout, 27), (1.0 + 2.0 ** -10) / 27.0, dtype=torch.float32)
    one = torch.ones(cout)
    return FwdProblem(geo, cout, stride, img8, (img8.float() / 255.0).contiguous(), w, one, one, O.reference(img8, w, stride))


# ---------------------------------------------------------------------------------------------------- weight gradient
WgradProblem = collections.namedtuple("WgradProblem", "geo cout stride u8 dtype field img dy old n dw A_dw P")


@functools.lru_cache(maxsize=None)
def wgrad_problem(geo_id, cout, stride, u8, dt, field, keep_patches=True):
    """field `random`: the forward problem's image, dy ~ 0.1 randn rounded to storage.  field `exact`: pixels 0..15 (uint8, or float p / 256),
    dy in {-1, 0, 1}.  old: the non-zero dw the launch accumulates onto.  P: the fp64 patches (dropped for the large case)"""
    geo, dtype = BY_ID[geo_id], DTYPES[dt]
    Ho, Wo = out_hw(geo, stride)
    g = torch.Generator().manual_seed(_seed(geo, cout, stride, field == "exact") + 11)
    if field == "exact":
        p = torch.randint(0, 16, (geo.B, 3, geo.H, geo.W), dtype=torch.uint8, generator=g)
        img = p if u8 else (p.float() / 256.0).contiguous()
        dy = torch.randint(-1, 2, (geo.B, cout, Ho, Wo), generator=g).float()
        O.assert_exact_field(img, dy, stride)
    else:
        f = fwd_problem(geo_id, cout, stride)
        img = f.img8 if u8 else f.imgf
        dy = O.store(0.1 * torch.randn(geo.B, cout, Ho, Wo, generator=g), dtype).float()
    old = (0.5 * torch.randn(cout, 27, generator=g)).contiguous()
    r = O.reference(img, None, stride, dy, forward=False)
    return WgradProblem(geo, cout, stride, u8, dtype, field, img, dy, old, r.n, r.dw, r.A_dw, r.P if keep_patches else None)


def wgrad_bound(p, sum_then_scale):
    """(target, bound) of dw after the launch.  The exact-field bound holds for a float image on any kernel, for a uint8 image only
    where the sum-then-scale kernel runs"""
    if p.field == "exact" and (not p.u8 or sum_then_scale):
        return O.dw_bound_exact(p.dw, p.A_dw, p.old)
    return O.dw_bound(p.n, p.dw, p.A_dw, p.old)


# ---------------------------------------------------------------------------------------------------- fused BatchNorm-backward apply
FUSED = [(gid, co, s) for gid in ("6x300", "7x520") for co, s in ((32, 1), (32, 2), (16, 2))]
FUSED_SLOTS = [1, 4, 16, 5]                    # 5: the scalar tail of the 4-wide replica fold
FusedProblem = collections.namedtuple("FusedProblem", "geo cout stride img8 da yraw scale mean rstd s1 s2 old_dw old_dg old_db P n")


@functools.lru_cache(maxsize=None)
def fused_problem(geo_id, cout, stride):
    """inputs distributed like those of tests/test_gpu_stem.py's fused test: da ~ 0.2 randn, yraw ~ 1.3 randn + 0.2 (bf16), mean / rstd of
    yraw in fp32, scale = (0.5 + rand) * rstd"""
    geo = BY_ID[geo_id]
    Ho, Wo = out_hw(geo, stride)
    g = torch.Generator().manual_seed(_seed(geo, cout, stride) + 23)
    img8 = torch.randint(0, 256, (geo.B, 3, geo.H, geo.W), dtype=torch.uint8, generator=g)
    da = (torch.randn(geo.B, cout, Ho, Wo, generator=g) * 0.2).bfloat16().float()
    yraw = (torch.randn(geo.B, cout, Ho, Wo, generator=g) * 1.3 + 0.2).bfloat16().float()
    mean = yraw.mean((0, 2, 3))
    rstd = (yraw.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    scale = (torch.rand(cout, generator=g) + 0.5) * rstd
    xhat = (yraw.double() - mean.double().view(1, -1, 1, 1)) * rstd.double().view(1, -1, 1, 1)
    s1, s2 = da.double().sum((0, 2, 3)), (da.double() * xhat).sum((0, 2, 3))
    old_dw = (0.5 * torch.randn(cout, 27, generator=g)).contiguous()
    old_dg, old_db = torch.full((cout,), 0.25), torch.full((cout,), -0.5)
    P = O.patches(O.image_values(img8), stride)
    return FusedProblem(geo, cout, stride, img8, da, yraw, scale, mean, rstd, s1, s2, old_dw, old_dg, old_db, P, geo.B * Ho * Wo)


def fused_red(p, slots):
    """[slots, 2, C] fp64: the two reduction sums spread unevenly over the replicas, as a fused data-gradient epilogue leaves them"""
    g = torch.Generator().manual_seed(slots)
    wts = torch.rand(slots, generator=g).double() ** 2 + 0.01
    wts /= wts.sum()
    red = torch.empty(slots, 2, p.cout, dtype=torch.float64)
    red[:, 0] = wts.view(-1, 1) * p.s1
    red[:, 1] = wts.view(-1, 1) * p.s2
    return red


def fused_ref(p, red):
    return O.fused_reference(p.da, p.yraw, p.scale, p.mean, p.rstd, red)


# ---------------------------------------------------------------------------------------------------- sentinel-framed buffers
SENTINEL = 1984.0                  # representable in bf16 and fp16
SENTINEL_U8 = 198
PAD_C = 16                         # padding channels of an output row
GUARD_ROWS = 4


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Buf:
    """a channels-last tensor [B, H, W, C] as the channel slice [off : off + C] of rows of `ld` elements, between guard rows, all of it
    filled with the sentinel; `shift` moves the base by that many elements (a misaligned base); .t is what the kernels get"""

    def __init__(self, B, H, W, C, dtype, ld=None, off=0, shift=0, device="cuda"):
        ld = ld or C + PAD_C
        n, g = B * H * W * ld, GUARD_ROWS * ld + shift
        self.flat = torch.full((g + n + GUARD_ROWS * ld,), SENTINEL, dtype=dtype, device=device)
        self.t = self.flat[g:g + n].view(B, H, W, ld)[..., off:off + C]
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        m[g:g + n].view(B, H, W, ld)[..., off:off + C] = True
        self.inside = m
        self.ld = ld
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
        a, b = _bits(self.flat.cpu()), _bits(self.before.cpu())
        out = torch.ones_like(self.inside) if everything else ~self.inside
        assert torch.equal(a[out], b[out]), "%d elements that must stay as they were have been written" % int((a[out] != b[out]).sum())

    def assert_untouched(self):
        self.assert_outside_untouched(everything=True)


class Flat:
    """a contiguous tensor of any shape between two guards of 64 sentinel elements, its base moved by `shift` elements"""

    def __init__(self, src, shift=0, device="cuda", fill=None):
        n = src.numel()
        sent = SENTINEL_U8 if src.dtype == torch.uint8 else SENTINEL
        self.flat = torch.full((64 + shift + n + 64,), sent, dtype=src.dtype, device=device)
        self.t = self.flat[64 + shift:64 + shift + n].view(src.shape)
        self.t.copy_(src if fill is None else torch.full_like(src, fill))
        m = torch.zeros(self.flat.numel(), dtype=torch.bool)
        m[64 + shift:64 + shift + n] = True
        self.inside = m
        self.before = None

    arm = Buf.arm
    assert_outside_untouched = Buf.assert_outside_untouched
    assert_untouched = Buf.assert_untouched
