"""The depthwise-convolution case matrix shared by tests/test_dwconv_reference.py (CPU: the fp64 reference and its bounds)
and tests/test_gpu_dwconv_elements.py (GPU: csrc/dwconv.hip held to them), with the inputs and the cached references.

Geometry of the LDS-tiled kernels (dwconv_tile_kernel, dwconv_wgrad_tile_kernel): CV = C / 8 channel vectors in
groups = ceil(CV / 8) groups of CT = ceil(CV / groups); output tiles of TH x 16 pixels, TH = (256 / CT) / 4:
    CT   1   2   3   4   5   6   7   8
    TH  64  32  21  16  12  10   9   8
The generic kernels take CVB = min(32, pow2 >= CV) channel vectors per workgroup and 256 / CVB pixel lanes.
"""
import collections
import functools

import torch

from oracle import dwconv as O

Case = collections.namedtuple("Case", "id B C H W k s pad slots ops view")

# ops: f forward, d data gradient, w weight gradient.  slots: BatchNorm-statistics replicas of the forward (0 = no statistics).
# view: x and dy are channel slices [8 : 8 + C] of a buffer with ld = C + 24 (outputs always have ld = C + 16; the weight gradient
# takes dy as [16 : 16 + C] of ld = C + 40): ldx != ldy in every op.  Tiled, row-strip and row-per-pixel weight gradients all have view cases.
# Every weight-gradient case keeps n = B*Ho*Wo <= 2048 (tests/test_dwconv_reference.py: a single lost pixel stays visible).
CASES = [
    # ---- stride 1, k = 3 | 5: the LDS-tiled kernels for bf16 / fp16, the generic and the row kernel (strip path) for fp32
    Case("c8_k3p1_66x17", 1, 8, 66, 17, 3, 1, 1, 1, "fdw", False),      # CT 1, TH 64: 2 x 2 tiles, ragged both ways, W = 17
    Case("c24_k5p2_23x17", 1, 24, 23, 17, 5, 1, 2, 3, "fdw", True),     # CT 3, TH 21 (4 idle threads): 2 x 2 ragged tiles
    Case("c56_k3p1_10x16", 2, 56, 10, 16, 3, 1, 1, 0, "fdw", False),    # CT 7, TH 9: W = 16 is exactly one tile, 2 tile rows
    Case("c64_k5p1_9x3", 2, 64, 9, 3, 5, 1, 1, 1, "fdw", True),         # CT 8; k 5 with pad 1 (DepthwiseSeparableConv2d): Wo = 1, W < 4, pad' = 3
    Case("c72_k3p1_1x17", 2, 72, 1, 17, 3, 1, 1, 3, "fdw", False),      # two groups of CT 5, the second partly filled; H = 1
    Case("c184_k3p1_1x1", 3, 184, 1, 1, 3, 1, 1, 1, "fdw", True),       # three groups, CT 8, the last partly filled; 1 x 1
    Case("c264_k5p0_6x21", 1, 264, 6, 21, 5, 1, 0, 1, "fdw", False),    # five groups of CT 7; pad 0 (pad' = 4), data gradient 2 tiles wide
    Case("c8_k3p0_5x20", 2, 8, 5, 20, 3, 1, 0, 0, "fdw", True),         # pad 0 at k 3 (pad' = 2)
    Case("c16_k5p2_35x33", 1, 16, 35, 33, 5, 1, 2, 3, "fdw", False),    # CT 2, TH 32: 2 x 3 tiles, several tiles per image
    Case("c4_k3p1_7x9", 2, 4, 7, 9, 3, 1, 1, 1, "fdw", True),           # fp32 only: one float4 vector
    # ---- stride 2: generic forward, dwconv_s2_dgrad_kernel data gradient (bf16), row weight gradient per-pixel path
    Case("c12_k5p2s2_9x8", 1, 12, 9, 8, 5, 2, 2, 3, "fdw", False),      # fp32 only, three float4 vectors; Hi odd, Wi even
    Case("c264_k3p1s2_9x12", 1, 264, 9, 12, 3, 2, 1, 1, "fdw", True),   # CVB 32: second channel block with ONE active vector; Hi odd, Wi even
    Case("c24_k3p0s2_8x10", 2, 24, 8, 10, 3, 2, 0, 0, "fdw", False),    # pad 0, Hi and Wi even: the last row AND column get no gradient
    Case("c8_k3p2s2_6x5", 1, 8, 6, 5, 3, 2, 2, 1, "fdw", True),         # pad 2 at k 3; Hi even, Wi odd
    Case("c72_k5p2s2_11x10", 2, 72, 11, 10, 5, 2, 2, 3, "fdw", False),  # k 5; Hi odd, Wi even
    Case("c16_k5p0s2_10x10", 1, 16, 10, 10, 5, 2, 0, 1, "fdw", True),   # k 5 pad 0: the last row and column get no gradient
    Case("c8_k5p1s2_9x12", 1, 8, 9, 12, 5, 2, 1, 0, "fdw", False),      # k 5 pad 1 (pad' parity differs from pad 2)
    # ---- the generic kernels at the other kernel sizes and strides; row weight gradient <T, 1> and <T, 7>
    Case("c24_k3p1s3_12x11", 2, 24, 12, 11, 3, 3, 1, 1, "fdw", True),   # stride 3: one tap per input pixel; the last row gets no gradient
    Case("c72_k1_5x9", 2, 72, 5, 9, 1, 1, 0, 1, "fdw", False),          # k 1
    Case("c8_k2p1_6x7", 1, 8, 6, 7, 2, 1, 1, 3, "fd", True),            # k 2 (no weight-gradient kernel for even k)
    Case("c16_k4p1_9x8", 1, 16, 9, 8, 4, 1, 1, 1, "fd", False),         # k 4
    Case("c24_k7p3_9x17", 1, 24, 9, 17, 7, 1, 3, 3, "fdw", True),       # k 7
    Case("c8_k7p3_60x5", 2, 8, 60, 5, 7, 1, 3, 0, "w", False),          # row kernel: 120 image rows over 109 workgroup rows (two rows in some)
    Case("c264_k1_683x1", 3, 264, 683, 1, 1, 1, 0, 1, "f", False),      # generic forward: 2049 image rows over 2048 workgroup rows; W = 1
    # ---- persistent tiled weight gradient with more tiles than workgroups per channel group (planes < tiles)
    Case("c960_k5p2_9x17", 9, 960, 9, 17, 5, 1, 2, 0, "w", False),      # 15 groups, 36 tiles, 18 workgroups each: n = 1377
    Case("c520_k3p1_2x17", 30, 520, 2, 17, 3, 1, 1, 0, "w", True),      # 9 groups, 60 tiles, 30 workgroups each: n = 1020
]
BY_ID = {c.id: c for c in CASES}

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}


def dtypes_of(case, op):
    """storage types an op of this case runs in: fp32 needs C % 4, the 16-bit types C % 8; fp16 is the inference type (forward)"""
    out = []
    if case.C % 8 == 0:
        out.append("bf16")
    out.append("f32")
    if case.C % 8 == 0 and op == "f":
        out.append("f16")
    return out


def matrix(op):
    return [(c.id, dt) for c in CASES if op in c.ops for dt in dtypes_of(c, op)]


def dead_tail(c):
    """(rows, columns) at the end of the conv input that no output pixel reads: their data gradient is exactly 0.  The window of the
    last output pixel ends (Hi + 2 pad - k) % s short of the padded input; what exceeds the padding is real input"""
    return (max(0, (c.H + 2 * c.pad - c.k) % c.s - c.pad), max(0, (c.W + 2 * c.pad - c.k) % c.s - c.pad))


def out_hw(c):
    return O.out_size(c.H, c.k, c.s, c.pad), O.out_size(c.W, c.k, c.s, c.pad)


Problem = collections.namedtuple("Problem", "case dtype x w dy old ref")


@functools.lru_cache(maxsize=None)
def problem(case_id, dt):
    """inputs (fp32 tensors holding storage-representable values; asymmetric random weights) and the fp64 reference; computed
    once, shared, never modified"""
    c, dtype = BY_ID[case_id], DTYPES[dt]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    Ho, Wo = out_hw(c)
    x = O.store(torch.randn(c.B, c.C, c.H, c.W, generator=g), dtype).float()
    w = (torch.randn(c.k * c.k, c.C, generator=g) / c.k).contiguous()
    dy = O.store(torch.randn(c.B, c.C, Ho, Wo, generator=g), dtype).float()
    old = O.store(torch.randn(c.B, c.C, c.H, c.W, generator=g), dtype).float()      # what the accumulate form adds onto
    return Problem(c, dtype, x, w, dy, old, O.reference(x, w, dy, c.k, c.s, c.pad))


# ---- the constant field: x = 1, every weight (1 + 2^-10) / k^2.  The accumulator is ~ 1 + 2^-10 and stores as 1.0 in bf16, so
# statistics taken from the STORED values are off by ~ 1e-3 relative: 15 x the s1 bound, 33 x the s2 bound at 2 x 16 x 17 x 23
CONST_SHAPE = (2, 16, 17, 23)


@functools.lru_cache(maxsize=None)
def const_problem(k=3, stride=1):
    B, C, H, W = CONST_SHAPE
    x = torch.ones(B, C, H, W)
    w = torch.full((k * k, C), (1.0 + 2.0 ** -10) / (k * k), dtype=torch.float32)
    c = Case("const", B, C, H, W, k, stride, k // 2, 1, "f", False)
    return Problem(c, torch.bfloat16, x, w, None, None, O.reference(x, w, None, k, stride, k // 2))


# ---- normalise + activation on load (DykDwDesc.pre): z = dtype(act(scale * u + shift))
ACTS = ["relu", "relu6", "hard-swish", "leaky", "linear", "mish"]


def act_fn(name):
    F = torch.nn.functional
    return {"relu": F.relu, "relu6": F.relu6, "hard-swish": F.hardswish, "leaky": lambda t: F.leaky_relu(t, 0.1),
            "linear": lambda t: t, "mish": F.mish}[name]


def pre_inputs(C, B, H, W, seed):
    """raw conv output u (bf16 values), scale, shift: scale * u + shift spans both signs and exceeds 6; act(shift) is far from 0,
    so padding the NORMALISED tensor with anything but 0 shows at every border"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    scale = 2.5 + torch.rand(C, generator=g)
    shift = 1.25 + 0.5 * torch.rand(C, generator=g)
    return u, scale, shift
