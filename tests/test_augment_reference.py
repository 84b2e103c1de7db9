"""What holds the yardstick of dyk_augment_pairs (tests/augment_ref.py) and the host half (build_utils/augment.py,
dyk.functional.augment_pairs) on the CPU: the hand-worked cases of the rule against literals, branch coverage of the case
matrix by named cases, twelve wrong kernels each flagged by a named case (and one that provably cannot be), the draws, matrices,
rectangles, tables and labels of the host functions against a restatement that cites the reference lines, the reference's
signatures, the refusals of the C entry and the descriptor layout.  No GPU: the launch itself is tests/test_gpu_augment.py.
Nothing here is pinned against cv2: there is none to run; agreement with it is derived, not measured."""
import ctypes
import inspect
import math
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img8():
    return (np.arange(64, dtype=np.uint8).reshape(8, 8) * 3 + 7)


def _warp1(img, M, out_size=None):
    """one plane through the rule under the forward matrix M"""
    src = np.stack([img, img, img])[None]
    ov, _ = R.augment(src, src, minv=R.invert(M)[None], out_size=out_size)
    assert np.array_equal(ov[0, 0], ov[0, 1]) and np.array_equal(ov[0, 0], ov[0, 2])
    return ov[0, 0]


# ---------------------------------------------------------------------------------------------- the rule, by hand
def test_identity_is_a_copy_and_a_null_matrix_is_the_identity():
    img = _img8()
    assert np.array_equal(_warp1(img, np.eye(3)), img)
    src = np.stack([img, img, img])[None]
    assert np.array_equal(R.augment(src, src)[0][0, 0], img)
    assert np.array_equal(R.invert(np.eye(3)), [1, 0, 0, 0, 1, 0])


def test_integer_translation_is_a_shifted_copy_in_a_zero_frame():
    img = _img8()
    out = _warp1(img, AC.shift(2, 1))
    want = np.zeros_like(img)
    want[1:, 2:] = img[:7, :6]
    assert np.array_equal(out, want)
    assert out[3].tolist() == [0, 0, 55, 58, 61, 64, 67, 70]         # row 2 of the image (7 + 3 * 16 = 55 ...) moved right by two


def test_half_pixel_translation_is_the_rounded_mean_of_two_neighbours():
    img = _img8()
    out = _warp1(img, AC.shift(0.5, 0))
    a, b = img[:, :-1].astype(int), img[:, 1:].astype(int)
    assert np.array_equal(out[:, 1:], (a * 512 + b * 512 + 512) >> 10)
    assert out[0].tolist() == [4, 9, 12, 15, 18, 21, 24, 27]         # (0 + 7 + 1) >> 1 = 4, (7 + 10 + 1) >> 1 = 9, (10 + 13 + 1) >> 1 ...


def test_border_minus_two_is_the_centre_crop():
    img = _img8()
    assert np.array_equal(_warp1(img, AC.shift(-2, -2), (4, 4)), img[2:6, 2:6])


def test_rotation_by_90_degrees_about_4_4_is_rot90_one_row_down():
    img = _img8()
    out = _warp1(img, AC.rot(90, 1.0, 4, 4))
    assert not out[0].any()                                          # source column 8 does not exist
    assert np.array_equal(out[1:], np.rot90(img)[:7])


def test_inversion_follows_the_order_of_the_rule():
    M = np.array([[0.9, 0.2, 3.0], [-0.1, 1.1, -2.0]])
    D = 1.0 / (0.9 * 1.1 - 0.2 * -0.1)
    m0, m1, m3, m4 = 1.1 * D, 0.2 * -D, -0.1 * -D, 0.9 * D
    want = [m0, m1, -m0 * 3.0 - m1 * -2.0, m3, m4, -m3 * 3.0 - m4 * -2.0]
    assert R.invert(M).tolist() == want
    from dyk.functional import invert_affine
    assert invert_affine(M) == want
    for bad in (np.zeros((2, 3)), [[1, 2, 0], [2, 4, 0]], [[np.nan, 0, 0], [0, 1, 0]], [[1, 0, np.inf], [0, 1, 0]]):
        with pytest.raises(ValueError):
            invert_affine(bad)


def test_division_tables_and_one_colour_by_hand():
    sdiv, hdiv = R.div_tables()
    assert sdiv[0] == 0 and hdiv[0] == 0 and sdiv[1] == 255 << 12 and hdiv[1] == 122880
    assert sdiv[200] == 5222 and hdiv[150] == 819 and sdiv[255] == 4096 and hdiv[255] == 482
    # (200, 100, 50): v = 200, diff = 150; s = (150 * 5222 + 2048) >> 12 = 191; h = (50 * 819 + 2048) >> 12 = 10
    one = lambda *c: [np.array([t]) for t in c]
    h, s, v = R.rgb_to_hsv(*one(200, 100, 50))
    assert (int(h[0]), int(s[0]), int(v[0])) == (10, 191, 200)
    assert [int(t[0]) for t in R.hsv_to_rgb(h, s, v)] == [200, 100, 50]
    # a negative hue wraps: (200, 50, 100) -> h = (-50 * 819 + 2048) >> 12 = -10 -> 170
    h, s, v = R.rgb_to_hsv(*one(200, 50, 100))
    assert (int(h[0]), int(s[0]), int(v[0])) == (170, 191, 200)


def test_primaries_greys_black_and_white_survive_the_round_trip_and_a_random_colour_need_not():
    cols = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)]
    cols += [(g, g, g) for g in range(256)]
    c = np.array(cols).T
    h, s, v = R.rgb_to_hsv(c[0], c[1], c[2])
    assert h[:6].tolist() == [0, 60, 120, 30, 90, 150] and s[:6].tolist() == [255] * 6
    back = np.stack(R.hsv_to_rgb(h, s, v))
    assert np.array_equal(back, c)
    rnd = np.random.RandomState(5).randint(0, 256, size=(3, 4096))
    back = np.stack(R.hsv_to_rgb(*R.rgb_to_hsv(rnd[0], rnd[1], rnd[2])))
    worst = int(np.abs(back - rnd).max())
    assert 1 <= worst <= 5, worst                                    # the rule, not a bug: hue has 180 steps


# ---------------------------------------------------------------------------------------------- coverage and mutants
COUNTER_CASE = {
    "rects_plain": "id_8x8", "rects_listed": "canvas4_mid", "rect_unused_slot": "batch3_picked", "rect_clipped_to_canvas": "canvas_clipped",
    "rect_skipped_outside_source": "rect_outside_source", "warp_null": "flip_alone_w10", "warp_matrix": "general_9x13",
    "tap_negative": "edges_9x13", "tap_outside_every_rect": "canvas4_low", "quad_in_one_rect": "canvas4_mid",
    "quad_straddles_rects": "canvas4_seams", "quad_partly_empty": "canvas4_low", "fraction_zero": "shift_8x8",
    "fraction_nonzero": "half_8x8", "jitter_none": "flip_alone_w12", "hsv_v_is_r": "hsv_identity_table", "hsv_v_is_g": "hsv_identity_table",
    "hsv_v_is_b": "hsv_identity_table", "hsv_h_wrapped": "hsv_identity_table", "hsv_grey": "hsv_identity_table", "hsv_exact_tie": "hsv_exact_tie",
    "hsv_sector_0": "hsv_hyp_gains", "hsv_sector_1": "hsv_hyp_gains", "hsv_sector_2": "hsv_hyp_gains", "hsv_sector_3": "hsv_hyp_gains",
    "hsv_sector_4": "hsv_hyp_gains", "hsv_sector_5": "hsv_hyp_gains", "flip_none": "id_8x8", "flip_yes": "flip_alone_w10",
    "flip_no": "flip_alone_w10"}

MUTANT_CASE = {
    "truncate": "half_8x8", "replicate_border": "shift_8x8", "no_plus_16": "general_9x13", "div_not_shift": "edges_9x13",
    "no_h_plus_180": "hsv_identity_table", "sector_row_permuted": "hsv_hyp_gains", "lut0_for_all": "batch3_plain",
    "l_wrong_matrix": "batch3_plain", "flip_source_side": "flip_warp_9x13", "swap_HoWo": "to_11x10", "seam_first_rect": "canvas4_seams",
    "round_half_away": "hsv_exact_tie"}


@pytest.mark.parametrize("counter", R.COUNTER_NAMES)
def test_every_counter_is_hit_by_a_named_case(counter):
    assert set(COUNTER_CASE) == set(R.COUNTER_NAMES)
    R.COUNTERS.clear()
    AC.run_ref(COUNTER_CASE[counter])
    assert R.COUNTERS[counter] > 0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_wrong_kernel_is_flagged_by_a_named_case(mutant):
    assert set(MUTANT_CASE) == set(R.MUTANTS) and len(R.MUTANTS) >= 10
    name = MUTANT_CASE[mutant]
    ov, ol = AC.run_ref(name, mutant)
    rv, rl = AC.reference(name)
    assert not (np.array_equal(ov, rv) and np.array_equal(ol, rl)), "%s passes %s" % (mutant, name)
    if mutant == "l_wrong_matrix":
        assert np.array_equal(ov, rv)                            # the visible stream is right: only a test of BOTH outputs sees it


def test_hue_branch_order_cannot_matter():
    """`v == g` tested before `v == r` is not a wrong kernel: on a tie r == g == v both branches give diff (g - b = diff,
    b - r + 2 diff = diff), on g == b == v both give 3 diff.  Held on every pair of ties."""
    lv = np.arange(256)
    a, b = np.meshgrid(lv, lv, indexing="ij")
    for r, g, bl in ((a, a, b), (b, a, a), (a, b, a)):
        assert np.array_equal(R.rgb_to_hsv(r, g, bl)[0], R.rgb_to_hsv(r, g, bl, mutant="g_before_r")[0])
    assert all(np.array_equal(x, y) for n in ("hsv_identity_table", "hsv_hyp_gains") for x, y in zip(AC.run_ref(n, "g_before_r"), AC.reference(n)))


def test_exact_ties_exist_in_the_final_rounding():
    """Half-away instead of half-even in clip(rint(x * 255.f)) is a wrong kernel only if some (h, s, v) gives x * 255.f exactly
    k + 0.5.  A search over all 180 x 256 x 256 triples finds such ties -- (1, 15, 255) gives green = 240.5 -- so
    `round_half_away` is among the mutants and the case hsv_exact_tie flags it."""
    s, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    s, v = s.reshape(-1), v.reshape(-1)
    R.COUNTERS.clear()
    for h in range(0, 180):
        R.hsv_to_rgb(np.full_like(s, h), s, v)
    assert R.COUNTERS["hsv_exact_tie"] > 0
    one = lambda *c: [np.array([t]) for t in c]
    assert [int(t[0]) for t in R.hsv_to_rgb(*one(1, 15, 255))] == [255, 240, 240]                            # 240.5 -> 240, the even one
    assert [int(t[0]) for t in R.hsv_to_rgb(*one(1, 15, 255), mutant="round_half_away")] == [255, 241, 240]


# ---------------------------------------------------------------------------------------------- the host half
class _Recorder:
    """stands in for dyk.functional.augment_pairs: keeps the parameters, returns blank outputs of the right shape"""

    def __init__(self):
        self.calls = []

    def __call__(self, v, l, matrices=None, rects=None, canvas=None, out_size=None, luts=None, flip=None, out=None):
        self.calls.append(dict(matrices=matrices, rects=rects, canvas=canvas, out_size=out_size, luts=luts, flip=flip, out=out))
        B = next((len(a) for a in (matrices, rects, luts, flip) if a is not None), v.shape[0])
        size = tuple(out_size) if out_size is not None else (tuple(canvas) if canvas is not None else tuple(v.shape[2:]))
        z = torch.zeros((B, 3) + size, dtype=torch.uint8)
        return z, z.clone()


@pytest.fixture
def recorder(monkeypatch):
    from dyk import functional as F
    rec = _Recorder()
    monkeypatch.setattr(F, "augment_pairs", rec)
    return rec


def _restated_matrix(rows, cols, degrees, translate, scale, shear, border):
    """kaist_dataset.py:428-444: R from getRotationMatrix2D(angle, centre (cols/2, rows/2), scale), T with the x shift scaled by
    the height (rows) and the y shift by the width, S with the two tangents; M = S @ T @ R"""
    a = random.uniform(-degrees, degrees)
    s = random.uniform(1 - scale, 1 + scale)
    tx = random.uniform(-translate, translate)
    ty = random.uniform(-translate, translate)
    sh0 = random.uniform(-shear, shear)
    sh1 = random.uniform(-shear, shear)
    Rm = AC.rot(a, s, cols / 2, rows / 2)
    T = AC.shift(tx * rows + border, ty * cols + border)
    S = np.array([[1, math.tan(sh0 * math.pi / 180), 0], [math.tan(sh1 * math.pi / 180), 1, 0], [0, 0, 1]])
    return S @ T @ Rm, s


def _restated_labels(labels, M, s, width, height):
    """kaist_dataset.py:452-477, box by box"""
    out = []
    for c, x1, y1, x2, y2 in labels:
        pts = [M @ np.array([x, y, 1.0]) for x, y in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
        xs, ys = [p[0] for p in pts], [p[1] for p in pts]
        nx1, nx2 = min(max(min(xs), 0), width), min(max(max(xs), 0), width)
        ny1, ny2 = min(max(min(ys), 0), height), min(max(max(ys), 0), height)
        w, h = nx2 - nx1, ny2 - ny1
        ar = max(w / (h + 1e-16), h / (w + 1e-16))
        if w > 4 and h > 4 and w * h / ((x2 - x1) * (y2 - y1) * s + 1e-16) > 0.2 and ar < 10:
            out.append([c, nx1, ny1, nx2, ny2])
    return np.array(out, np.float64).reshape(-1, 5)


def _boxes(rng, n, W, H):
    x1, y1 = rng.uniform(0, W * 0.8, n), rng.uniform(0, H * 0.8, n)
    return np.stack([rng.randint(0, 3, n).astype(np.float64), x1, y1, x1 + rng.uniform(2, W * 0.4, n), y1 + rng.uniform(2, H * 0.4, n)], 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_affine_draws_matrix_and_labels(recorder, seed):
    from build_utils import augment as A
    H, W, border = 20, 28, -3
    v = torch.zeros(3, H, W, dtype=torch.uint8)
    labels = _boxes(np.random.RandomState(seed), 9, W, H)
    random.seed(seed)
    M, s = _restated_matrix(H, W, 10, 0.1, 0.1, 0.1, border)
    nxt = random.random()
    random.seed(seed)
    ov, ol, got = A.random_affine(v, v.clone(), labels.copy(), border=border)
    assert random.random() == nxt                                 # six draws, no more
    call = recorder.calls[0]
    assert np.array_equal(call["matrices"][0], M[:2]) and tuple(call["out_size"]) == (H + 2 * border, W + 2 * border)
    assert tuple(ov.shape) == (3, H + 2 * border, W + 2 * border)
    want = _restated_labels(labels, M, s, W + 2 * border, H + 2 * border)
    assert 0 < len(want) and np.allclose(got, want, rtol=0, atol=1e-9) and got.shape == want.shape
    # a CPU tensor comes back as one, in its dtype
    random.seed(seed)
    _, _, got_t = A.random_affine(v, v.clone(), torch.from_numpy(labels).float(), border=border)
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.float32 and got_t.shape == want.shape


def test_random_affine_with_nothing_to_do_returns_the_images_themselves(recorder):
    from build_utils import augment as A
    v, l = torch.zeros(3, 8, 8, dtype=torch.uint8), torch.ones(3, 8, 8, dtype=torch.uint8)
    ov, ol, lab = A.random_affine(v, l, np.array([[0, 1.0, 1.0, 7.0, 7.0]]), degrees=0, translate=0, scale=0, shear=0)
    assert ov is v and ol is l and not recorder.calls
    assert np.array_equal(lab, [[0, 1.0, 1.0, 7.0, 7.0]])


def test_hsv_tables_follow_the_reference(recorder):
    from build_utils import augment as A
    v = torch.zeros(3, 8, 8, dtype=torch.uint8)
    np.random.seed(11)
    r = np.random.uniform(-1, 1, 3) * [0.0138, 0.678, 0.36] + 1          # kaist_dataset.py:493
    nxt = np.random.rand()
    np.random.seed(11)
    l = v.clone()
    assert A.augment_hsv(v, l, 0.0138, 0.678, 0.36) is None
    assert np.random.rand() == nxt
    call = recorder.calls[0]
    want = R.hsv_tables(r)
    assert np.array_equal(call["luts"][0], want) and call["out"][0].data_ptr() == v.data_ptr() and call["out"][1].data_ptr() == l.data_ptr()
    # by hand: entry 255 of the hue table is trunc(255 * r0 mod 180); saturation and value clip at 255 before the cast
    assert int(want[0, 255]) == int((255 * r[0]) % 180) and int(want[1, 255]) == int(min(255 * r[1], 255)) and want.max() <= 255
    assert int(want[0].max()) <= 179


def _paste(xr, yr, s, sizes, srcs):
    """kaist_dataset.py:232-255 acted out: paste coordinate images into a 2s x 2s array with the reference's slices; each
    cell holds (source + 1, y, x), 0 = background"""
    def spans(centre, n, before):
        """one axis: (canvas slice, source slice).  A tile before the centre lies against it with its far end and loses its
        near end at the canvas edge; a tile after it starts at the centre and loses its far end"""
        if before:
            lo = max(centre - n, 0)
            return slice(lo, centre), slice(n - (centre - lo), n)
        hi = min(centre + n, 2 * s)
        return slice(centre, hi), slice(0, hi - centre)

    cv = np.zeros((2 * s, 2 * s, 3), np.int64)
    pads = []
    for slot, j in enumerate(srcs):
        h, w = sizes[j]
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([np.full((h, w), j + 1), yy, xx], 2)
        (cx, sx), (cy, sy) = spans(xr, w, slot % 2 == 0), spans(yr, h, slot < 2)
        cv[cy, cx] = img[sy, sx]
        pads.append((cx.start - sx.start, cy.start - sy.start))
    return cv, pads


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_mosaic_rectangles_and_labels(recorder, seed):
    from build_utils import augment as A
    B, h, w, s = 5, 12, 16, 16
    rng = np.random.RandomState(seed)
    labs = [np.concatenate([rng.randint(0, 2, (n, 1)), rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.2, 0.5, (n, 2))], 1) for n in (2, 0, 3, 1, 2)]
    hyp = {"degrees": 5, "translate": 0.05, "scale": 0.2, "shear": 2}
    index = seed % B
    random.seed(seed)
    xr, yr = [int(random.uniform(s * 0.5, s * 1.5)) for _ in range(2)]                   # :224
    srcs = [index] + [random.randint(0, B - 1) for _ in range(3)]                        # :226
    M, sc = _restated_matrix(2 * s, 2 * s, 5, 0.05, 0.2, 2, -s // 2)                     # :279-284
    nxt = random.random()
    random.seed(seed)
    v = torch.zeros(B, 3, h, w, dtype=torch.uint8)
    ov, ol, got = A.mosaic(v, v.clone(), labs, index, img_size=s, hyp=hyp)
    assert random.random() == nxt
    call = recorder.calls[0]
    assert tuple(call["canvas"]) == (2 * s, 2 * s) and tuple(call["out_size"]) == (s, s) and tuple(ov.shape) == (3, s, s)
    assert np.array_equal(call["matrices"][0], M[:2])
    # the rectangles give the canvas the reference pastes: coordinate images through augment_ref's canvas()
    want_cv, pads = _paste(xr, yr, s, [(h, w)] * B, srcs)
    yy, xx = np.mgrid[0:h, 0:w]
    coord = np.stack([np.stack([np.full((h, w), j + 1), yy, xx]) for j in range(B)]).astype(np.uint8)
    ys, xs = np.mgrid[0:2 * s, 0:2 * s]
    got_cv, _ = R.canvas(coord, call["rects"][0], 0, 2 * s, 2 * s, ys, xs)
    assert np.array_equal(got_cv.transpose(1, 2, 0), want_cv)
    assert [tuple(r[5:7]) for r in call["rects"][0].tolist()] == pads and call["rects"].dtype == np.int32
    # labels: :258-272, then random_affine's
    l4 = []
    for j, (pw, ph) in zip(srcs, pads):
        for c, x, y, bw, bh in labs[j]:
            l4.append([c, w * (x - bw / 2) + pw, h * (y - bh / 2) + ph, w * (x + bw / 2) + pw, h * (y + bh / 2) + ph])
    l4 = np.array(l4).reshape(-1, 5)
    l4[:, 1:] = np.clip(l4[:, 1:], 0, 2 * s)
    want = _restated_labels(l4, M, sc, s, s)
    assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-9)


def restated_batch(t, B, H, W, s, hyp, mosaic, flip=True):
    """B calls of the reference's __getitem__ (kaist_dataset.py:321-369) in order, on the current state of `random` and
    `np.random`; t fp64 [n,6] -> (forward matrices [B,2,3], rects [B,4,8] or None, tables [B,3,256], flips [B], targets [m,6],
    (Ho, Wo))"""
    Ms, luts, flips, out, rects = [], [], [], [], []
    gains = [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]]
    aff = (hyp["degrees"], hyp["translate"], hyp["scale"], hyp["shear"])
    for b in range(B):
        if mosaic:
            xr, yr = [int(random.uniform(s * 0.5, s * 1.5)) for _ in range(2)]           # :224
            srcs = [b] + [random.randint(0, B - 1) for _ in range(3)]                    # :226
            _, pads = _paste(xr, yr, s, [(H, W)] * B, srcs)
            rec = AC.quad_rects(xr, yr, s, H, W, srcs)
            assert [tuple(r[5:7]) for r in rec] == pads
            rects.append(rec)
            lab = []
            for j, (pw, ph) in zip(srcs, pads):                                          # :258-272
                for _, c, x, y, bw, bh in t[t[:, 0] == j]:
                    lab.append([c, W * (x - bw / 2) + pw, H * (y - bh / 2) + ph, W * (x + bw / 2) + pw, H * (y + bh / 2) + ph])
            lab = np.array(lab).reshape(-1, 5)
            lab[:, 1:] = np.clip(lab[:, 1:], 0, 2 * s)
            M, sc = _restated_matrix(2 * s, 2 * s, *aff, -s // 2)                        # :279-284
            Ho = Wo = 2 * s + 2 * (-s // 2)
        else:
            lab = np.array([[c, W * (x - bw / 2), H * (y - bh / 2), W * (x + bw / 2), H * (y + bh / 2)]
                            for _, c, x, y, bw, bh in t[t[:, 0] == b]]).reshape(-1, 5)
            M, sc = _restated_matrix(H, W, *aff, 0)                                      # :343-347
            Ho, Wo = H, W
        lab = _restated_labels(lab, M, sc, Wo, Ho)
        Ms.append(M[:2])
        luts.append(R.hsv_tables(np.random.uniform(-1, 1, 3) * gains + 1))               # :348, :493
        xywh = np.stack([lab[:, 0], (lab[:, 1] + lab[:, 3]) / 2 / Wo, (lab[:, 2] + lab[:, 4]) / 2 / Ho, (lab[:, 3] - lab[:, 1]) / Wo,
                         (lab[:, 4] - lab[:, 2]) / Ho], 1)                               # :354-358
        f = bool(flip) and random.random() < 0.5                                         # :365
        if f:
            xywh[:, 1] = 1 - xywh[:, 1]
        flips.append(int(f))
        out.append(np.concatenate([np.full((len(xywh), 1), b), xywh], 1))
    return np.stack(Ms), (np.array(rects, np.int32) if mosaic else None), np.stack(luts), flips, np.concatenate(out), (Ho, Wo)


def batch_targets(B, n=7, seed=4):
    rng = np.random.RandomState(seed)
    t = np.concatenate([np.sort(rng.randint(0, B, (n, 1)), 0), rng.randint(0, 2, (n, 1)), rng.uniform(0.3, 0.7, (n, 2)), rng.uniform(0.3, 0.5, (n, 2))], 1)
    return torch.from_numpy(t).float()


BATCH_HYP = {"degrees": 3, "translate": 0.05, "scale": 0.1, "shear": 1, "hsv_h": 0.0138, "hsv_s": 0.678, "hsv_v": 0.36}


@pytest.mark.parametrize("mosaic", [False, True], ids=["plain", "mosaic"])
def test_augment_batch_draws_what_one_getitem_per_image_draws(recorder, mosaic):
    from build_utils import augment as A
    B, H, W, s = 3, 24, 32, 32
    targets = batch_targets(B)
    random.seed(9)
    np.random.seed(9)
    want_M, want_rects, want_lut, want_flip, want_t, (Ho, Wo) = restated_batch(targets.numpy().astype(np.float64), B, H, W, s, BATCH_HYP, mosaic)
    nxt = (random.random(), np.random.rand())
    random.seed(9)
    np.random.seed(9)
    v = torch.zeros(B, 3, H, W, dtype=torch.uint8)
    ov, ol, got = A.augment_batch(v, v.clone(), targets, BATCH_HYP, mosaic=mosaic, img_size=s)
    assert (random.random(), np.random.rand()) == nxt
    assert len(recorder.calls) == 1                                  # one launch for the batch
    call = recorder.calls[0]
    assert np.array_equal(call["matrices"], want_M) and np.array_equal(call["luts"], want_lut)
    assert call["flip"].tolist() == want_flip and tuple(ov.shape) == (B, 3, Ho, Wo)
    if mosaic:
        assert np.array_equal(call["rects"], want_rects) and tuple(call["canvas"]) == (2 * s, 2 * s)
    else:
        assert call["rects"] is None
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == want_t.shape and len(want_t) > 0
    assert np.allclose(got.numpy(), want_t, rtol=0, atol=1e-6)


def test_augment_batch_with_zero_hyp_passes_no_matrix_and_keeps_the_labels(recorder):
    from build_utils import augment as A
    targets = torch.tensor([[0, 1, 0.5, 0.5, 0.25, 0.5], [1, 0, 0.25, 0.75, 0.25, 0.375]])      # both above the 4-pixel filter of :474
    hyp = {"degrees": 0, "translate": 0, "scale": 0, "shear": 0, "hsv_h": 0.0138, "hsv_s": 0.678, "hsv_v": 0.36}
    random.seed(1)
    v = torch.zeros(2, 3, 16, 32, dtype=torch.uint8)
    _, _, got = A.augment_batch(v, v.clone(), targets, hyp)
    call = recorder.calls[0]
    assert call["matrices"] is None and call["rects"] is None and call["luts"].shape == (2, 3, 256)
    want = targets.clone()
    want[:, 2] = torch.where(torch.from_numpy(call["flip"].astype(bool))[want[:, 0].long()], 1 - want[:, 2], want[:, 2])
    assert torch.allclose(got, want, rtol=0, atol=1e-6)
    _, _, got = A.augment_batch(v, v.clone(), targets, hyp, flip=False)
    assert recorder.calls[1]["flip"] is None and torch.allclose(got, targets, rtol=0, atol=1e-6)


def test_signatures_equal_the_reference():
    from build_utils import augment as A
    from dyk import functional as F
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    # kaist_dataset.py:408 and :482
    assert sig(A.random_affine) == [("v_img", E), ("l_img", E), ("labels", ()), ("degrees", 10), ("translate", 0.1), ("scale", 0.1),
                                    ("shear", 0.1), ("border", 0)]
    assert sig(A.augment_hsv) == [("v_img", E), ("l_img", E), ("h_gain", 0.5), ("s_gain", 0.5), ("v_gain", 0.5)]
    assert sig(A.mosaic) == [("v_imgs", E), ("l_imgs", E), ("labels_per_image", E), ("index", E), ("img_size", None), ("hyp", None)]
    assert sig(A.augment_batch) == [("v_imgs", E), ("l_imgs", E), ("targets", E), ("hyp", E), ("mosaic", False), ("flip", True), ("img_size", None)]
    assert sig(F.augment_pairs) == [("v", E), ("l", E), ("matrices", None), ("rects", None), ("canvas", None), ("out_size", None),
                                    ("luts", None), ("flip", None), ("out", None)]
    img = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="no CPU fallback"):
        F.augment_pairs(img, img.clone())
    with pytest.raises(TypeError):
        F.augment_pairs(img.numpy(), img.numpy())
    import build_utils
    assert not os.path.exists(os.path.join(os.path.dirname(build_utils.__file__), "kaist_dataset.py"))   # that name is the reference's


# ---------------------------------------------------------------------------------------------- the C ABI
def _desc(L, **kw):
    """no GPU here: a launch would fail with DYK_ERR_HIP (-2), not DYK_ERR_ARG (-1).  The addresses are never dereferenced."""
    a = dict(src_v=0x100000, src_l=0x200000, dst_v=0x300000, dst_l=0x400000, N=2, B=2, H=8, W=8, Hc=8, Wc=8, Ho=8, Wo=8, rects=None,
             minv=None, luts=None, flip=None)
    a.update(kw)
    return L.DykAugmentDesc(**a)


def test_abi_symbol_and_refused_arguments():
    from dyk import lib as L
    h = L.load()
    assert h.dyk_abi_version() == 5 and L.ABI_VERSION == 5
    assert hasattr(h, "dyk_augment_pairs") and "dyk_augment_pairs" in L.SIGNATURES
    assert h.dyk_augment_pairs(None, None) == -1
    for rows in (0, -1, 65):                                          # the probe's entry: rows per workgroup within 1..64
        assert h.dyk_augment_pairs_rows(ctypes.byref(_desc(L)), rows, None) == -1
    assert h.dyk_augment_pairs_rows(ctypes.byref(_desc(L, N=0)), 2, None) == -1
    refused = [{"src_v": None}, {"src_l": None}, {"dst_v": None}, {"dst_l": None}, {"N": 0}, {"B": 0}, {"H": 0}, {"W": 0}, {"Ho": 0},
               {"Wo": -1}, {"H": 16385}, {"Wo": 16385, "minv": 0x500000}, {"B": 3},                      # B > N without rects
               {"Ho": 4}, {"Wo": 12},                                                                    # no matrix: the output is the canvas
               {"rects": 0x500000, "Hc": 0}, {"rects": 0x500000, "Hc": 16, "Wc": 16},                    # ... 16 x 16 here, not 8 x 8
               {"dst_v": 0x100000, "minv": 0x500000}, {"dst_v": 0x100000, "rects": 0x500000}, {"dst_v": 0x100000, "flip": 0x500000},
               {"dst_v": 0x100010}, {"dst_v": 0x200000}, {"dst_l": 0x100000},                            # partial overlap; crossed streams
               {"dst_l": 0x300000}, {"dst_l": 0x300100},                                                 # the two outputs overlap
               {"dst_v": 0x100000, "N": 3}]                                                              # in place needs B == N
    for kw in refused:
        assert h.dyk_augment_pairs(ctypes.byref(_desc(L, **kw)), None) == -1, kw


def test_descriptor_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib as L
    cls = L.DykAugmentDesc
    names = [f[0] for f in cls._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){", 'printf("size %zu\\n", sizeof(DykAugmentDesc));']
    lines += ['printf("%s %%zu\\n", offsetof(DykAugmentDesc, %s));' % (n, n) for n in names]
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["size"]) == ctypes.sizeof(cls) == 96
    for n in names:
        assert int(out[n]) == getattr(cls, n).offset, n
    assert L.AUGMENT_MAX_SIZE == 16384
