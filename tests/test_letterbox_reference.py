"""What holds the yardstick of dyk_resize_pad_pairs (tests/letterbox_ref.py) itself, on the CPU: hand-worked cases for each
rule of include/dyk_hip.h, the letterbox geometry worked by hand from the reference's img_utils.py, and wrong kernels (the
`mutant=` forms) that must each be flagged by a named case of tests/letterbox_cases.py.  Nothing here is pinned against cv2:
there is none to run; the rule is derived from OpenCV's published 8-bit resize, not measured."""
import ctypes

import numpy as np
import pytest

import letterbox_cases as LC
import letterbox_ref as R

f32 = np.float32


def _img(vals):
    return np.asarray(vals, np.uint8)[None]                       # one plane [1,h,w]


# ------------------------------------------------------------------------------------------------ hand-worked pixel rules
@pytest.mark.parametrize("interp,h,w,nh,nw", [(R.LINEAR, 5, 7, 4, 5), (R.LINEAR, 5, 7, 11, 13), (R.AREA, 6, 8, 3, 4), (R.AREA, 9, 6, 3, 2),
                                              (R.AREA, 9, 7, 4, 5), (R.LINEAR, 8, 8, 4, 4), (R.AREA, 5, 7, 5, 7)])
def test_a_constant_image_stays_constant(interp, h, w, nh, nw):
    for val in (0, 1, 77, 254, 255):
        out = R.resize(np.full((1, h, w), val, np.uint8), nh, nw, interp)
        assert out.shape == (1, nh, nw) and (out == val).all(), (val, np.unique(out))


def test_identity_coefficients_give_the_source_back():
    S = np.random.RandomState(0).randint(0, 256, (3, 6, 9)).astype(np.uint8)
    # equal sizes: a copy by rule; and the LINEAR arithmetic itself at scale 1 (fx = fy = 0, a0 = b0 = 2048) returns S:
    assert np.array_equal(R.resize(S, 6, 9, R.LINEAR), S) and np.array_equal(R.resize(S, 6, 9, R.AREA), S)
    s, c0, c1 = R.linear_coeffs(9, 9, True)
    assert np.array_equal(s, np.arange(9)) and (c0 == 2048).all() and (c1 == 0).all()
    assert np.array_equal(R.resize_linear(S, 6, 9), S)
    assert np.array_equal(R.resize_area(S, 6, 9), S)            # integer factors 1 x 1: rn(sum * 1.f)


def test_one_block_in_each_area_form():
    # (i) 2 x 2 with sum % 4 == 2: (sum + 2) >> 2 rounds the half UP, rn(sum * 0.25f) to even
    blk = _img([[1, 2], [3, 4]])                                  # sum 10 -> 2.5
    assert R.resize(blk, 1, 1, R.AREA)[0, 0, 0] == 3
    assert R.resize(blk, 1, 1, R.AREA, mutant="area2_float")[0, 0, 0] == 2
    assert R.resize(blk, 1, 1, R.LINEAR)[0, 0, 0] == 3            # LINEAR at exactly 2 x is AREA
    # (i) another integer factor: 2 x 3 block, sum 21, one fp32 multiply by 1.f / 6 -> 3.5 -> 4 (half to even)
    blk = _img([[1, 2, 3], [4, 5, 6]])
    assert f32(21) * (f32(1) / f32(6)) == f32(3.5) and R.resize(blk, 1, 1, R.AREA)[0, 0, 0] == 4
    blk = _img([[13] * 7, [0] * 7])                               # 2 x 7, sum 91: 91 * (1.f / 14) = 6.5000005 -> 7 (exact 6.5 would give 6)
    assert f32(91) * (f32(1) / f32(14)) > f32(6.5) and R.resize(blk, 1, 1, R.AREA)[0, 0, 0] == 7
    # (ii) weighted: 3 -> 2 columns, scale 1.5: taps (0, 1/1.5), (1, .5/1.5) and (1, .5/1.5), (2, 1/1.5)
    taps = R.area_taps(3, 2)
    assert [[s for s, _ in t] for t in taps] == [[0, 1], [1, 2]]
    a, b = f32(1.0 / 1.5), f32(0.5 / 1.5)
    assert [[w for _, w in t] for t in taps] == [[a, b], [b, a]]
    row = _img([[30, 60, 90], [30, 60, 90], [30, 60, 90]])        # 3 x 3 -> 2 x 2
    out = R.resize(row, 2, 2, R.AREA)
    assert out.tolist() == [[[40, 80], [40, 80]]]                 # (30 + 60 / 2) / 1.5 = 40, (60 / 2 + 90) / 1.5 = 80
    # the last cell is cut to what is left of the source: 5 -> 2, scale 2.5, second cell [2.5, 5)
    assert [[s for s, _ in t] for t in R.area_taps(5, 2)] == [[0, 1, 2], [2, 3, 4]]


def test_vectorised_area_equals_the_scalar_loops():
    for name in ("shrink54_area_15x20", "steep_area_64", "area_one_axis", "area_w37"):
        c = LC.case(name)
        nh, nw, top, left, _ = c["geom"][0]
        S = c["v"][0]
        want = LC.reference(name)[0][0]
        ty, tx = R.area_taps(S.shape[1], nh), R.area_taps(S.shape[2], nw)
        for p in range(3):
            for y in range(nh):
                for x in range(nw):
                    assert R.area_pixel_scalar(S[p], ty[y], tx[x]) == want[p, top + y, left + x], (name, p, y, x)


def test_linear_by_hand():
    # 2 -> 4 columns, scale 0.5: fx = -0.25 (reset), 0.25, 0.75, 1.25 (sx = 1 = w - 1: reset)
    s, a0, a1 = R.linear_coeffs(2, 4, True)
    assert s.tolist() == [0, 0, 0, 1] and a0.tolist() == [2048, 1536, 512, 2048] and a1.tolist() == [0, 512, 1536, 0]
    # rows: no reset: sy = -1 with fy = 0.75 at the top, sy = 1 with fy = 0.25 at the bottom
    s, b0, b1 = R.linear_coeffs(2, 4, False)
    assert s.tolist() == [-1, 0, 0, 1] and b0.tolist() == [512, 1536, 512, 1536] and b1.tolist() == [1536, 512, 1536, 512]
    out = R.resize(_img([[0, 100], [200, 255]]), 4, 4, R.LINEAR)[0]
    # column 1 of row 1: D0 = 0 * 1536 + 100 * 512 = 51200, D1 = 200 * 1536 + 255 * 512 = 437760;
    # ((1536 * 3200) >> 16) + ((512 * 27360) >> 16) = 75 + 213 = 288; (288 + 2) >> 2 = 72
    assert out[1, 1] == 72
    assert out[0].tolist() == [0, 25, 75, 100]                    # the top row: both taps are row 0
    assert out[3, 3] == 255 and out[3, 0] == 200
    # the vertical form: >> 22 would give (1536 * 51200 + 512 * 437760 + 2^21) >> 22 = 72 here, and differs elsewhere
    D0, D1, b0, b1 = 10 * 2048, 11 * 2048, 1000, 1048           # 10.51: each product loses its fraction before the sum
    assert (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2 == 10 and (b0 * D0 + b1 * D1 + (1 << 21)) >> 22 == 11


def search_edge_sum(max_src=2, max_dst=6000):
    """the first (n_src, n_dst) with a right-edge column (sx >= n_src - 1 before the reset) whose unreset coefficients do not
    sum to 2048: there S * (a0 + a1) differs from the rule's S * 2048"""
    for n_src in range(1, max_src + 1):
        for n_dst in range(n_src + 1, max_dst):
            s, c0, c1 = R.linear_coeffs(n_src, n_dst, True, "no_edge_exception")
            if ((s >= n_src - 1) & (c0 + c1 != 2048)).any():
                return n_src, n_dst
    return None


def search_scale_pair(n_dst=8192, lo=4097):
    """the first odd n_src >= lo with 1 / (n_dst / n_src) != n_src / n_dst in fp64"""
    for n_src in range(lo, n_dst, 2):
        if R.axis_scale(n_src, n_dst) != n_src / n_dst:
            return n_src, n_dst
    return None


def test_the_right_edge_exception_on_a_column_where_a0_plus_a1_is_not_2048():
    n_src, n_dst = LC.EDGE_SUM
    assert (n_src, n_dst) == (1, 5463)
    s, c0, c1 = R.linear_coeffs(n_src, n_dst, True, "no_edge_exception")
    bad = np.nonzero((s >= n_src - 1) & (c0 + c1 != 2048))[0]
    assert len(bad) == 1 and c0[bad[0]] + c1[bad[0]] in (2047, 2049)
    s, c0, c1 = R.linear_coeffs(n_src, n_dst, True)              # the rule: fx = 0 there, and D = S * 2048 whatever a1 is
    assert c0[bad[0]] == 2048 and c1[bad[0]] == 0
    want, got = LC.reference("edge_sum"), LC.run_ref("edge_sum", "no_edge_exception")
    diff = np.nonzero(want[0] != got[0])
    assert len(diff[0]) > 0 and set(diff[3].tolist()) == {int(bad[0])}     # only that column


def test_the_hard_coded_search_results_are_what_the_searches_find():
    assert search_edge_sum(max_src=1) == LC.EDGE_SUM
    assert search_scale_pair(lo=5801) == LC.SCALE_PAIR          # (the first pair whose OUTPUT differs too; earlier ones differ only in the scale)


def test_scale_is_two_roundings():
    n_src, n_dst = LC.SCALE_PAIR
    assert (n_src, n_dst) == (5845, 8192)
    assert R.axis_scale(n_src, n_dst) != n_src / n_dst
    assert R.axis_scale(n_src, n_dst) == 1.0 / (8192.0 / 5845.0)
    assert abs(R.axis_scale(n_src, n_dst) - n_src / n_dst) < 2.3e-16         # one unit in the last place of 0.71
    assert R.axis_scale(640, 512) == 1.25 and R.axis_scale(512, 410) == 1.0 / (410.0 / 512.0)


def test_coefficients_round_half_to_even():
    s, c0, c1 = R.linear_coeffs(3, 2048, True)
    s2, h0, h1 = R.linear_coeffs(3, 2048, True, "half_away")
    mid = (s > 0) & (s < 2)
    assert ((c0 + c1)[mid] == 2048).all() and ((h0 + h1)[mid] == 2049).all()


# ------------------------------------------------------------------------------------------------ geometry by hand
def test_letterbox_geometry_by_hand():
    # 512 x 640 -> 512, auto: r = 0.8, new_unpad = (512, 410), dw = 0, dh = 102 % 64 = 38 -> 19: top 19, bottom 19
    ratio, pad, content, sides = R.letterbox_geometry((512, 640), 512, auto=True)
    assert ratio == (0.8, 0.8) and pad == (0.0, 19.0) and content == (410, 512) and sides == (19, 19, 0, 0)
    # auto=False: dh = 102 -> 51: top = round(50.9) = 51, bottom = round(51.1) = 51
    ratio, pad, content, sides = R.letterbox_geometry((512, 640), 512, auto=False)
    assert ratio == (0.8, 0.8) and pad == (0.0, 51.0) and content == (410, 512) and sides == (51, 51, 0, 0)
    # an odd difference: 409 rows (what load_image leaves: int(512 * 0.8)) -> dh = 51.5: top = round(51.4) = 51, bottom = round(51.6) = 52
    _, pad, content, sides = R.letterbox_geometry((409, 512), 512, auto=False, scale_up=False)
    assert pad == (0.0, 51.5) and content == (409, 512) and sides == (51, 52, 0, 0)
    # scale_up=False on a small image: r = min(4.0, 3.2) -> 1.0: only padded; dw = 312 -> 156, dh = 384 -> 192
    ratio, pad, content, sides = R.letterbox_geometry((128, 200), 512, auto=False, scale_up=False)
    assert ratio == (1.0, 1.0) and pad == (156.0, 192.0) and content == (128, 200) and sides == (192, 192, 156, 156)
    # with scale_up: r = 2.56 -> 512 x 328 (round(327.68))
    ratio, pad, content, sides = R.letterbox_geometry((128, 200), 512, auto=False, scale_up=True)
    assert ratio == (2.56, 2.56) and content == (328, 512) and pad == (0.0, 92.0) and sides == (92, 92, 0, 0)
    # the scale_fill quirk on new_shape = (H, W) = (320, 416) and a 100 x 200 image: ratio = (320 / 200, 416 / 100), and
    # new_unpad = (320, 416) read as (width, height): the image becomes 416 rows of 320 columns
    ratio, pad, content, sides = R.letterbox_geometry((100, 200), (320, 416), auto=False, scale_fill=True)
    assert ratio == (1.6, 4.16) and pad == (0.0, 0.0) and content == (416, 320) and sides == (0, 0, 0, 0)
    # under auto, scale_fill is never reached
    assert R.letterbox_geometry((100, 200), (320, 416), auto=True, scale_fill=True) == R.letterbox_geometry((100, 200), (320, 416), auto=True)


def test_product_geometry_equals_the_restatement():
    from build_utils import letterbox as LB
    for shape, new_shape, auto, fill, up in [((512, 640), 512, True, False, True), ((512, 640), 512, False, False, True),
                                             ((409, 512), 512, False, False, False), ((128, 200), 512, False, False, False),
                                             ((100, 200), (320, 416), False, True, True), ((375, 500), (416, 416), True, False, True),
                                             ((33, 77), (64, 96), False, False, True)]:
        got, want = LB._geometry(shape, new_shape, auto, fill, up), R.letterbox_geometry(shape, new_shape, auto, fill, up)
        assert got[0] == want[0] and tuple(float(t) for t in got[1]) == want[1] and got[2:] == want[2:], (shape, new_shape)
    assert LB._load_size(512, 640, 512, False) == ((409, 512), R.AREA)       # int(512 * 0.8) = 409
    assert LB._load_size(512, 640, 512, True) == ((409, 512), R.LINEAR)
    assert LB._load_size(512, 640, 640, False) == ((512, 640), R.LINEAR)      # r == 1: untouched
    assert LB._load_size(240, 320, 640, False) == ((480, 640), R.LINEAR)      # r > 1 is LINEAR in validation too


def test_letterbox_labels_by_hand():
    from build_utils import letterbox as LB
    x = np.array([[1, 0.5, 0.5, 0.25, 0.5]])
    out = LB.letterbox_labels(x, (0.8, 0.8), (0.0, 51.0), 640, 512)
    assert np.allclose(out, [[1, 0.8 * 640 * 0.375, 0.8 * 512 * 0.25 + 51, 0.8 * 640 * 0.625, 0.8 * 512 * 0.75 + 51]], rtol=0, atol=1e-12)
    assert LB.letterbox_labels(np.zeros((0, 5)), (1, 1), (0, 0), 4, 4).shape == (0, 5)


# ------------------------------------------------------------------------------------------------ the case matrix and the mutants
def test_the_case_matrix_covers_what_it_must():
    geoms = {n: LC.case(n) for n in LC.CASES}
    assert any(c["layout"] == "hwc_bgr" for c in geoms.values()) and any(c["layout"] == "chw" for c in geoms.values())
    assert any(tuple(c["color"]) != (0, 0, 0) for c in geoms.values())
    c = geoms["batch3_mixed"]
    assert len({a.shape for a in c["v"]}) == 3 and {g[4] for g in c["geom"]} == {R.LINEAR, R.AREA}
    c = geoms["pad_only_odd"]
    (nh, nw, top, left, _), (Ho, Wo) = c["geom"][0], c["out_size"]
    assert top != Ho - top - nh and left != Wo - left - nw
    s, _, _ = R.linear_coeffs(9, 22, False)
    assert s[0] == -1                                              # up_9x13: sy = -1 at the top
    s, _, _ = R.linear_coeffs(13, 31, True)
    assert (s + 1 >= 13).any()                                     # and columns with sx + 1 >= w
    assert max(len(t) for t in R.area_taps(64, 3)) >= 20          # the steep case: many taps
    for n in ("unstaged_area", "unstaged_area_int", "unstaged_linear"):
        c = geoms[n]
        h, w = c["v"][0].shape[1:] if c["layout"] == "chw" else c["v"][0].shape[:2]
        assert 3 * h * w * min(8, c["geom"][0][0]) // c["geom"][0][0] > 32768      # the rows behind one band exceed the LDS stage
    for n, c in geoms.items():
        shapes = [a.shape[1:] if c["layout"] == "chw" else a.shape[:2] for a in c["v"]]
        assert all(R.check(s, g, c["out_size"]) is None for s, g in zip(shapes, c["geom"])), n


def test_linear_at_2x_is_area_and_the_fixed_point_form_agrees():
    """at exactly 2 x every LINEAR coefficient is 1024, and (1024 * ((1024 * s) >> 4)) >> 16 is s exactly: the LINEAR arithmetic
    gives (sum + 2) >> 2 itself, so the `linear2x_not_switched` mutant is provably the same function; asserted, not flagged"""
    S = np.asarray(LC.case("exact2_lin")["v"][0])
    assert np.array_equal(R.resize(S, 6, 8, R.LINEAR), R.resize(S, 6, 8, R.AREA))
    assert np.array_equal(R.resize(S, 6, 8, R.LINEAR), ((S.astype(np.int32).reshape(3, 6, 2, 8, 2).sum(axis=(2, 4)) + 2) >> 2).astype(np.uint8))
    a, b = LC.reference("exact2_lin"), LC.run_ref("exact2_lin", "linear2x_not_switched")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


FLAGGED = [m for m in R.MUTANTS if m != "linear2x_not_switched"]


@pytest.mark.parametrize("mutant", FLAGGED)
def test_each_wrong_kernel_is_flagged_by_its_named_case(mutant):
    assert len(FLAGGED) >= 10
    name = LC.MUTANT_CASE[mutant]
    want, got = LC.reference(name), LC.run_ref(name, mutant)
    assert not (np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])), "%s is not flagged by %s" % (mutant, name)


def test_the_yardstick_refuses_what_the_rule_refuses():
    S = [np.zeros((3, 8, 8), np.uint8)]
    for geom, out in [((9, 8, 0, 0, R.AREA), (9, 8)), ((4, 9, 0, 0, R.AREA), (8, 9)), ((4, 4, 5, 0, 0), (8, 8)), ((4, 4, 0, -1, 0), (8, 8)),
                      ((0, 4, 0, 0, 0), (8, 8)), ((4, 4, 0, 0, 2), (8, 8)), ((4, 4, 0, 0, 0), (8, 16385))]:
        with pytest.raises(ValueError):
            R.resize_pad(S, S, [geom], out)


def test_the_entry_refuses_before_the_launch():
    """DYK_ERR_ARG comes from the host records, before any device work: it can be checked without a GPU"""
    from dyk import lib as L
    h = L.load()
    assert h.dyk_resize_pad_pairs(None, None) == -1
    src, dst = ctypes.create_string_buffer(3 * 8 * 8), ctypes.create_string_buffer(2 * 3 * 8 * 8 + 16)
    sa, da = ctypes.addressof(src), ctypes.addressof(dst)

    def call(rec=None, **kw):
        r = dict(src_v=sa, src_l=sa, h=8, w=8, nh=4, nw=4, top=0, left=0, interp=0)
        r.update(rec or {})
        recs = (L.DykResizePadRec * 1)(L.DykResizePadRec(**r))
        d = dict(recs=ctypes.addressof(recs), recs_host=ctypes.addressof(recs), dst_v=da, dst_l=da + 3 * 8 * 8, B=1, Ho=8, Wo=8, layout=0)
        d.update(kw)
        return h.dyk_resize_pad_pairs(ctypes.byref(L.DykResizePadDesc(**d)), None)

    for kw in (dict(recs=None), dict(recs_host=None), dict(dst_v=None), dict(dst_l=None), dict(B=0), dict(Ho=0), dict(Wo=0), dict(Wo=16385),
               dict(layout=2), dict(layout=-1), dict(dst_l=da + 3 * 8 * 8 - 1), dict(dst_v=sa)):
        assert call(**kw) == -1, kw
    for rec in (dict(src_v=None), dict(src_l=None), dict(h=0), dict(w=16385), dict(nh=0), dict(nw=0), dict(interp=2), dict(interp=-1),
                dict(top=-1), dict(top=5), dict(left=5), dict(nh=9, nw=8, interp=1), dict(nh=8, nw=9, interp=1), dict(nh=9, interp=1)):
        assert call(rec) == -1, rec
