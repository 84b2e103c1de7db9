"""The yardstick of dyk_clahe / dyk_cutout_rects (tests/clahe_ref.py) and the host half of build_utils.snowflake, without a GPU.

The yardstick is a restatement of OpenCV's published 8-bit CLAHE; no OpenCV is installed where this project runs, so what holds
it to the algorithm is here: the hand-worked tables of two constant tiles, the properties every table must have, and the
coverage of every branch of the rule by a named case of tests/clahe_cases.py.  tests/test_gpu_clahe.py then holds the kernels
to the yardstick bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clahe_cases as CC
import clahe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# branch of the rule -> a named case that must go through it
COVERED_BY = {
    "pad_none": "8x8_g2", "pad_both": "10x13_g4", "pad_forced_on_divisible_axis": "10x12_g4",
    "clip_zero": "clip0", "clip_floored_to_1": "clip0.01", "residual_zero": "clip40",
    "step_one": "const_tile256", "step_above_one": "const_tile16", "saturate_255": "6x14_g2",
    "band_left": "33x47_g8", "band_right": "33x47_g8", "band_top": "33x47_g16x3", "band_bottom": "33x47_g16x3",
}


def test_every_branch_of_the_rule_is_reached_by_a_named_case():
    assert sorted(COVERED_BY) == sorted(clahe_ref.COUNTER_NAMES)
    for counter, name in COVERED_BY.items():
        CC.reference(name)
        assert CC.COVERAGE[name].get(counter, 0) > 0, "%s does not reach %s: %s" % (name, counter, CC.COVERAGE[name])


def test_geometry_of_the_named_cases():
    g = clahe_ref.geometry
    assert g(8, 8, 2, 2) == (0, 0, 4, 4)
    assert g(10, 13, 4, 4) == (3, 2, 4, 3)
    assert g(10, 12, 4, 4) == (4, 2, 4, 3)               # W divisible: a full extra tiles_x
    assert g(5, 5, 4, 4) == (3, 3, 2, 2)
    assert g(5, 5, 9, 9) == (4, 4, 1, 1)                 # pad == n - 1: the last extended index reads 2(n-1) - (2n-2) = 0
    assert g(33, 47, 16, 3) == (1, 3, 3, 12)
    assert g(96, 97, 4, 4) == (3, 4, 25, 25)
    assert g(512, 640, 4, 4) == (0, 0, 160, 128)
    assert clahe_ref._reflect(8, 5) == 0 and clahe_ref._reflect(5, 5) == 3 and clahe_ref._reflect(4, 5) == 4
    for H, W, (tx, ty) in CC.REFUSED:
        with pytest.raises(ValueError):
            g(H, W, tx, ty)


def test_constant_tile_of_16_pixels_by_hand():
    """8 x 8 of value 100, grid (2, 2): area 16, clip = max(int(1.0 * 16 / 256), 1) = 1.  The histogram is 16 in bin 100:
    clipped = 15, batch 0, residual 15, step = 256 // 15 = 17, so bins 0, 17, ..., 238 get +1 and bin 100 keeps 1.
    lutScale = 255 / 16 = 15.9375 (exact); prefix sum p -> rint(15.9375 p), 127.5 going to the even 128."""
    by_prefix = [0, 16, 32, 48, 64, 80, 96, 112, 128, 143, 159, 175, 191, 207, 223, 239, 255]
    want = np.array([by_prefix[min(i // 17 + 1, 15) + (1 if i >= 100 else 0)] for i in range(256)], np.uint8)
    dst, luts = CC.reference("const_tile16")
    assert luts.shape == (1, 4, 256)
    for t in range(4):
        assert np.array_equal(luts[0, t], want)
    assert want[100] == 112 and np.all(dst == 112)


def test_constant_tile_of_256_pixels_by_hand():
    """32 x 32 of value 100, grid (2, 2): area 256, clip 1, clipped = 255, residual 255, step 1: bins 0..254 get +1, so bin 100
    holds 2 and bin 255 nothing.  lutScale = 255/256: prefix p -> rint(p - p/256) = p below 128, 128 at p = 128 (127.5 to
    even), p - 1 above."""
    prefix = [i + 1 if i < 100 else min(i + 2, 256) for i in range(256)]
    want = np.array([p if p <= 128 else p - 1 for p in prefix], np.uint8)
    dst, luts = CC.reference("const_tile256")
    for t in range(4):
        assert np.array_equal(luts[0, t], want)
    assert want[100] == 102 and want[126] == 128 and want[127] == 128 and want[255] == 255
    assert np.all(dst == 102)


def test_tables_are_monotonic_and_end_at_255_but_clahe_is_not_the_identity():
    changed = 0
    for name in CC.SMALL:
        dst, luts = CC.reference(name)
        src = CC.case(name)["imgs"]
        assert dst.shape == src.shape and dst.dtype == np.uint8
        assert luts.shape == (src.shape[0], CC.case(name)["grid"][0] * CC.case(name)["grid"][1], 256)
        assert np.all(np.diff(luts.astype(np.int32), axis=-1) >= 0), name
        assert np.all(luts[..., 255] == 255), name                   # the prefix sum ends at the tile area
        changed += int((dst != src).sum())
    assert changed > 0
    # without a clip limit a table is the plain equalisation: rint(255 cdf)
    src = CC.case("clip0")["imgs"][0]
    cdf = np.cumsum(np.bincount(src[:32, :32].ravel(), minlength=256))
    assert np.array_equal(CC.reference("clip0")[1][0, 0], np.rint(np.float32(cdf) * (np.float32(255.0) / np.float32(1024))).astype(np.uint8))


def test_every_wrong_kernel_is_flagged_by_its_named_case():
    assert sorted(CC.WITNESS) == sorted(clahe_ref.MUTANTS + ("inclusive_ends",))
    for m in CC.WITNESS:
        assert CC.flagged(m), "%s is not told from the rule by %s" % (m, CC.WITNESS[m])


def test_cutout_yardstick_is_numpy_slicing():
    for name in CC.CUT_CASES:
        c = CC.cut_case(name)
        want = np.array(c["imgs"], copy=True)
        for p in range(want.shape[0]):
            for xmin, ymin, xmax, ymax in c["rects"][p // c["planes_per_set"]]:
                if xmin < 0 or ymin < 0:                              # a negative slice start counts from the end in numpy
                    xmin, ymin = max(xmin, 0), max(ymin, 0)
                want[p, ymin:max(ymax, 0), xmin:max(xmax, 0)] = c["value"]
        got = clahe_ref.cutout(c["imgs"], c["rects"], c["planes_per_set"], c["value"])
        assert np.array_equal(got, want), name
        assert not np.array_equal(got, c["imgs"])


# ---------------------------------------------------------------------------------------------- build_utils.snowflake, host half
def test_random_cut_box_against_a_hand_restatement():
    from build_utils.snowflake import random_cut_box
    for seed, (w, h, n, step) in enumerate([(512, 640, 25, 16), (64, 80, 10, 32), (9, 7, 5, 16)]):
        r = np.random.RandomState(seed).rand(n, 2)
        want = np.zeros((n, 4))
        for i in range(n):
            x, y = r[i, 0] * (w - 1), r[i, 1] * (h - 1)
            want[i] = [np.floor(x), np.floor(y), np.floor(min(max(x + step - 1, 0), w - 1)), np.floor(min(max(y + step - 1, 0), h - 1))]
        np.random.seed(seed)
        got = random_cut_box(w, h, n, step)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.random.rand() == np.random.RandomState(seed).rand(2 * n + 1)[-1]        # exactly one rand(n, 2) was drawn
        assert np.all(got[:, 2] <= w - 1) and np.all(got[:, 3] <= h - 1) and np.all(got[:, 2:] - got[:, :2] <= step - 1 + 1)


def test_cover_iou_on_three_hand_worked_pairs():
    from build_utils.snowflake import cover_iou
    # three boxes, no side above M = 3: 2x2 of a 4x4 label -> 4/16; 1x1 -> 1/16; disjoint -> 0
    got = cover_iou(np.array([[0., 0., 4., 4.]]), np.array([[1., 1., 3., 3.], [3., 3., 9., 9.], [10., 10., 12., 12.]]))
    assert np.array_equal(got, [[0.25, 0.0625, 0.0]])
    # the clip at M bites: two boxes, the 5 x 5 overlap counts as 2 x 2 -> 4/100 (0.25 without the reference's quirk)
    got = cover_iou(np.array([[0., 0., 10., 10.]]), np.array([[0., 0., 5., 5.], [20., 20., 30., 30.]]))
    assert np.array_equal(got, [[0.04, 0.0]])
    # label area floored at 1: a 0.5 x 0.5 label inside one box -> 0.25 / 1
    got = cover_iou(np.array([[2., 2., 2.5, 2.5], [0., 0., 2., 8.]]), np.array([[0., 0., 16., 16.]]))
    assert np.array_equal(got, [[0.25], [1.0 / 16.0]])                # second label: sides clipped to 1 x 1 of its 16


def test_snowflake_has_the_reference_names_and_needs_a_device():
    import inspect
    import torch
    from build_utils import snowflake as S
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(S.random_cut_box) == [("w", E), ("h", E), ("n", 10), ("step", 32)]
    assert sig(S.cover_iou) == [("box1", E), ("box2", E)]
    assert sig(S.clahe_image) == [("v_img", E), ("l_img", E), ("clip_limit", 1.0), ("tile_grid_size", (4, 4))]
    want = [("labels", E), ("xywh", True), ("clahe", True), ("label_thr", 0.35), ("n_thr", 6), ("step", 16), ("n_snow", 25),
            ("clip_limit", 1.0), ("grid_size", (4, 4))]
    assert sig(S.snowflake_cutout) == [("v_img", E), ("l_img", E)] + want
    assert sig(S.snowflake_batch) == [("v_imgs", E), ("l_imgs", E), ("targets", E)] + want[1:]
    from dyk import functional as F
    img = torch.zeros(3, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="no CPU fallback"):
        F.clahe(img)
    with pytest.raises(TypeError, match="no CPU fallback"):
        F.cutout(img, torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(TypeError):
        S.clahe_image(img, img)
    with pytest.raises(TypeError):
        F.clahe(img.numpy())


# ---------------------------------------------------------------------------------------------- the C ABI
def _desc(L, H=8, W=8, grid=(2, 2), planes=1, src=64, dst=64, lut=4096, clip=1.0):
    """no GPU here: a launch would fail with DYK_ERR_HIP (-2), not DYK_ERR_ARG (-1).  The addresses are never dereferenced."""
    return L.DykClaheDesc(src=src, dst=dst, lut=lut, planes=planes, H=H, W=W, tiles_x=grid[0], tiles_y=grid[1], clip_limit=clip)


def test_abi_symbols_and_refused_arguments():
    from dyk import lib as L
    h = L.load()
    assert h.dyk_abi_version() == 5 and L.ABI_VERSION == 5
    for name in ("dyk_clahe", "dyk_clahe_ws_bytes", "dyk_cutout_rects"):
        assert hasattr(h, name) and name in L.SIGNATURES
    assert h.dyk_clahe(None, None) == -1
    for planes, tx, ty in [(1, 1, 1), (6, 4, 4), (96, 4, 4), (7, 16, 3), (3, 16, 16)]:
        assert h.dyk_clahe_ws_bytes(planes, tx, ty) == planes * tx * ty * 256
    for planes, tx, ty in [(0, 4, 4), (1, 0, 4), (1, 4, 17), (-1, 4, 4)]:
        assert h.dyk_clahe_ws_bytes(planes, tx, ty) == -1
    for H, W, grid in CC.REFUSED:
        assert h.dyk_clahe(ctypes.byref(_desc(L, H, W, grid)), None) == -1, (H, W, grid)
    for kw in ({"src": None}, {"dst": None}, {"lut": None}, {"planes": 0}, {"planes": -3}, {"planes": 1 << 24, "H": 512, "W": 640, "grid": (4, 4)}):
        assert h.dyk_clahe(ctypes.byref(_desc(L, **kw)), None) == -1, kw
    cut = lambda img=64, planes=3, H=8, W=8, rects=128, nrect=2, pps=3, value=0: h.dyk_cutout_rects(img, planes, H, W, rects, nrect, pps, value, None)
    for kw in ({"img": None}, {"planes": 0}, {"H": 0}, {"W": 0}, {"rects": None}, {"nrect": -1}, {"pps": 0}, {"value": 256}, {"value": -1}):
        assert cut(**kw) == -1, kw
    assert cut(nrect=0) == 0 and cut(nrect=0, rects=None) == 0       # nothing to cut: no launch


def test_clahe_descriptor_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib as L
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dyk_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu\\n", sizeof(DykClaheDesc), offsetof(DykClaheDesc, lut), offsetof(DykClaheDesc, tiles_y),'
                   ' offsetof(DykClaheDesc, clip_limit)); return 0;}')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    D = L.DykClaheDesc
    assert got == [ctypes.sizeof(D), D.lut.offset, D.tiles_y.offset, D.clip_limit.offset] == [56, 16, 40, 48]
