"""dyk_augment_pairs on the GPU (csrc/augment.hip, dyk.functional.augment_pairs, build_utils.augment) against the plain numpy
yardstick tests/augment_ref.py: uint8 outputs, so every image comparison is bit for bit -- there is no tolerance on pixels
anywhere in this file.  Shapes and rules: tests/augment_cases.py; what holds the yardstick itself:
tests/test_augment_reference.py.  Nothing here is pinned against cv2: there is none to run."""
import ctypes
import random

import numpy as np
import pytest
import torch

import augment_cases as AC
import augment_ref as R
from test_augment_reference import BATCH_HYP, _paste, _restated_labels, _restated_matrix, batch_targets, restated_batch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
TAIL = 64


def _lib():
    from dyk import lib as L
    return L, L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _framed(nbytes, lead):
    """a device buffer of `nbytes` between `lead` and TAIL sentinel bytes -> (whole, view of the payload).  lead = 256 keeps the
    payload aligned for the dword stores; an odd lead takes the byte stores"""
    whole = torch.full((lead + nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[lead:lead + nbytes]


def _frame_intact(whole, lead):
    return bool((whole[:lead] == SENTINEL).all()) and bool((whole[-TAIL:] == SENTINEL).all())


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # (a copy: the cases are read-only)


def _run(name, aligned=True):
    """the case through the C ABI on framed buffers -> (rc, dst_v, dst_l, frames intact, sources unchanged)"""
    L, h = _lib()
    c = AC.case(name)
    N, _, H, W = c["src_v"].shape
    B = c["B"]
    Hc, Wc = c["canvas"] if c["rects"] is not None else (H, W)
    Ho, Wo = c["out_size"] if c["out_size"] is not None else (Hc, Wc)
    leads = (256, 256, 256, 256) if aligned else (3, 1, 5, 7)
    bufs = []
    for k, a in enumerate((c["src_v"], c["src_l"])):
        w, p = _framed(a.size, leads[k])
        p.copy_(torch.from_numpy(np.array(a)).reshape(-1))
        bufs.append((w, p))
    if c["in_place"]:
        bufs += bufs[:2]
    else:
        bufs += [_framed(B * 3 * Ho * Wo, leads[2]), _framed(B * 3 * Ho * Wo, leads[3])]
    rects, mi, luts, flip = _dev(c["rects"]), _dev(AC.minv(c)), _dev(c["luts"]), _dev(c["flip"])
    ptr = lambda t: None if t is None else t.data_ptr()
    d = L.DykAugmentDesc(src_v=bufs[0][1].data_ptr(), src_l=bufs[1][1].data_ptr(), dst_v=bufs[2][1].data_ptr(), dst_l=bufs[3][1].data_ptr(),
                         N=N, B=B, H=H, W=W, Hc=Hc, Wc=Wc, Ho=Ho, Wo=Wo, rects=ptr(rects), minv=ptr(mi), luts=ptr(luts), flip=ptr(flip))
    rc = h.dyk_augment_pairs(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    intact = all(_frame_intact(w, leads[k if not c["in_place"] else k % 2]) for k, (w, _) in enumerate(bufs))
    same = c["in_place"] or (np.array_equal(bufs[0][1].cpu().numpy().reshape(c["src_v"].shape), c["src_v"]) and
                             np.array_equal(bufs[1][1].cpu().numpy().reshape(c["src_l"].shape), c["src_l"]))
    shape = (B, 3, Ho, Wo)
    return rc, bufs[2][1].cpu().numpy().reshape(shape), bufs[3][1].cpu().numpy().reshape(shape), intact, same


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s differs in %d of %d bytes" % (what, int((got != want).sum()), want.size)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd_bases"])
@pytest.mark.parametrize("name", AC.SMALL)
def test_both_outputs_equal_the_yardstick_bit_for_bit(name, aligned):
    want_v, want_l = AC.reference(name)
    rc, ov, ol, intact, same = _run(name, aligned)
    assert rc == 0
    _equal(ov, want_v, "visible")
    _equal(ol, want_l, "lwir")
    assert intact and same


def test_full_size_batch_twice():
    """2 x 512 x 640 with every plain stage on: equal to the yardstick, and two runs give the same bytes"""
    want_v, want_l = AC.reference(AC.FULL)
    rc, ov, ol, intact, same = _run(AC.FULL)
    assert rc == 0 and intact and same
    _equal(ov, want_v, "visible")
    _equal(ol, want_l, "lwir")
    rc2, ov2, ol2, intact2, _ = _run(AC.FULL)
    assert rc2 == 0 and intact2 and np.array_equal(ov2, ov) and np.array_equal(ol2, ol)


@pytest.mark.parametrize("name", ["general_37x53", "canvas4_seams", "all_stages", "jitter_in_place_w13", "batch3_picked"])
def test_two_runs_give_identical_bytes(name):
    a, b = _run(name), _run(name, aligned=False)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", [n for n in AC.CASES if not AC.case(n)["raw"]])
def test_functional_augment_pairs_equals_the_yardstick(name):
    from dyk import functional as F
    c = AC.case(name)
    want_v, want_l = AC.reference(name)
    v, l = _dev(c["src_v"]), _dev(c["src_l"])
    ov, ol = F.augment_pairs(v, l, matrices=c["M"], rects=c["rects"], canvas=c["canvas"], out_size=c["out_size"], luts=c["luts"],
                             flip=c["flip"], out=(v, l) if c["in_place"] else None)
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    if c["in_place"]:
        assert ov.data_ptr() == v.data_ptr() and ol.data_ptr() == l.data_ptr()
    else:
        assert np.array_equal(v.cpu().numpy(), c["src_v"]) and np.array_equal(l.cpu().numpy(), c["src_l"])


def test_functional_augment_pairs_refuses_what_the_rule_refuses():
    from dyk import functional as F
    v = torch.zeros((2, 3, 8, 12), dtype=torch.uint8, device="cuda")
    l = torch.zeros_like(v)
    eye = np.stack([np.eye(3)[:2]] * 2)
    for bad in ([[1, 2, 0], [2, 4, 0]], [[np.nan, 0, 0], [0, 1, 0]], [[1, 0, 0], [0, np.inf, 0]]):
        with pytest.raises(ValueError):
            F.augment_pairs(v, l, matrices=np.stack([np.eye(3)[:2], np.array(bad, np.float64)]))
    with pytest.raises(ValueError, match="2\\^20"):
        F.augment_pairs(v, l, matrices=np.stack([AC.shift(2.0 ** 20 + 1, 0)[:2]] * 2))
    with pytest.raises(ValueError, match="2\\^20"):
        F.augment_pairs(v, l, matrices=np.stack([AC.rot(0, 1e-6, 0, 0)[:2]] * 2), out_size=(8, 16384))
    # every corner inside 2^20, but the column term m0 * (Wo - 1) alone is about 2^21: ad could reach the edge of int32
    edge = F.invert_affine([[(2.0 ** 21 - 4) / 11, 0, -(2.0 ** 20 - 1)], [0, 1, 0]])
    with pytest.raises(ValueError, match="across the output"):
        F.augment_pairs(v, l, matrices=np.stack([np.array(edge).reshape(2, 3)] * 2))
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, matrices=eye, out_size=(8, 16385))
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, out_size=(4, 12))                       # no matrix: the output is the canvas
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, matrices=eye[:1])                       # one parameter set for two images, no rects
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, rects=np.zeros((1, 4, 8), np.int32))    # no canvas
    rect = np.zeros((1, 4, 8), np.int32)
    rect[0, 0] = (0, 0, 12, 8, 2, 0, 0, 0)                            # source 2 of 2
    with pytest.raises(ValueError, match="outside"):
        F.augment_pairs(v, l, rects=rect, canvas=(8, 12))
    rect[0, 0] = (0, 0, 12, 8, 1, -1, 0, 0)                           # reads column 12 of 12
    with pytest.raises(ValueError, match="outside"):
        F.augment_pairs(v, l, rects=rect, canvas=(8, 12))
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, matrices=eye, out=(v, l))               # in place is for jitter alone
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, flip=[1, 0], out=(v, l))
    with pytest.raises(ValueError):
        F.augment_pairs(v, l, luts=np.zeros((2, 3, 255), np.uint8))
    with pytest.raises(TypeError):
        F.augment_pairs(v, l, luts=np.zeros((2, 3, 256), np.float32))
    with pytest.raises(TypeError):
        F.augment_pairs(v.float(), l.float())
    with pytest.raises(ValueError):
        F.augment_pairs(v, l[:1])
    with pytest.raises(ValueError):
        F.augment_pairs(v.permute(0, 1, 3, 2), l.permute(0, 1, 3, 2))
    assert not v.any() and not l.any()


# ---------------------------------------------------------------------------------------------- build_utils.augment
def _pair(seed, N, H, W):
    r = np.random.RandomState(seed)
    return r.randint(0, 256, (N, 3, H, W)).astype(np.uint8), r.randint(0, 256, (N, 3, H, W)).astype(np.uint8)


def test_random_affine_under_a_fixed_seed():
    from build_utils import augment as A
    H, W, border = 20, 28, -3
    sv, sl = _pair(1, 1, H, W)
    rng = np.random.RandomState(2)
    x1, y1 = rng.uniform(0, W * 0.6, 8), rng.uniform(0, H * 0.6, 8)
    labels = np.stack([np.zeros(8), x1, y1, x1 + rng.uniform(5, 12, 8), y1 + rng.uniform(5, 12, 8)], 1)
    random.seed(3)
    M, s = _restated_matrix(H, W, 10, 0.1, 0.1, 0.1, border)
    want_v, want_l = R.augment(sv, sl, minv=R.invert(M)[None], out_size=(H + 2 * border, W + 2 * border))
    want_lab = _restated_labels(labels, M, s, W + 2 * border, H + 2 * border)
    random.seed(3)
    ov, ol, lab = A.random_affine(_dev(sv[0]), _dev(sl[0]), labels.copy(), border=border)
    _equal(ov.cpu().numpy(), want_v[0], "visible")
    _equal(ol.cpu().numpy(), want_l[0], "lwir")
    assert lab.shape == want_lab.shape and len(lab) > 0 and np.allclose(lab, want_lab, rtol=0, atol=1e-9)
    v = _dev(sv[0])
    ov, _, _ = A.random_affine(v, _dev(sl[0]), degrees=0, translate=0, scale=0, shear=0)
    assert ov is v                                                    # nothing to do: the image itself, as the reference returns it


def test_augment_hsv_in_place_under_a_fixed_seed():
    from build_utils import augment as A
    sv, sl = _pair(4, 1, 11, 14)
    np.random.seed(5)
    tab = R.hsv_tables(np.random.uniform(-1, 1, 3) * [0.0138, 0.678, 0.36] + 1)
    want_v, want_l = R.augment(sv, sl, luts=tab[None])
    v, l = _dev(sv[0]), _dev(sl[0])
    np.random.seed(5)
    assert A.augment_hsv(v, l, 0.0138, 0.678, 0.36) is None
    _equal(v.cpu().numpy(), want_v[0], "visible")
    _equal(l.cpu().numpy(), want_l[0], "lwir")


def test_mosaic_under_a_fixed_seed():
    from build_utils import augment as A
    B, h, w, s = 4, 12, 16, 16
    sv, sl = _pair(6, B, h, w)
    rng = np.random.RandomState(7)
    labs = [np.concatenate([np.zeros((2, 1)), rng.uniform(0.3, 0.7, (2, 2)), rng.uniform(0.4, 0.6, (2, 2))], 1) for _ in range(B)]
    hyp = {"degrees": 5, "translate": 0.05, "scale": 0.2, "shear": 2}
    random.seed(8)
    xr, yr = [int(random.uniform(s * 0.5, s * 1.5)) for _ in range(2)]
    srcs = [2] + [random.randint(0, B - 1) for _ in range(3)]
    M, sc = _restated_matrix(2 * s, 2 * s, 5, 0.05, 0.2, 2, -s // 2)
    rects = np.array([AC.quad_rects(xr, yr, s, h, w, srcs)], np.int32)
    want_v, want_l = R.augment(sv, sl, 1, rects, (2 * s, 2 * s), R.invert(M)[None], (s, s))
    _, pads = _paste(xr, yr, s, [(h, w)] * B, srcs)
    l4 = np.array([[c, w * (x - bw / 2) + pw, h * (y - bh / 2) + ph, w * (x + bw / 2) + pw, h * (y + bh / 2) + ph]
                   for j, (pw, ph) in zip(srcs, pads) for c, x, y, bw, bh in labs[j]])
    l4[:, 1:] = np.clip(l4[:, 1:], 0, 2 * s)
    want_lab = _restated_labels(l4, M, sc, s, s)
    random.seed(8)
    ov, ol, lab = A.mosaic(_dev(sv), _dev(sl), labs, 2, img_size=s, hyp=hyp)
    _equal(ov.cpu().numpy(), want_v[0], "visible")
    _equal(ol.cpu().numpy(), want_l[0], "lwir")
    assert lab.shape == want_lab.shape and np.allclose(lab, want_lab, rtol=0, atol=1e-9)


@pytest.mark.parametrize("mosaic", [False, True], ids=["plain", "mosaic"])
def test_augment_batch_under_fixed_seeds(mosaic):
    from build_utils import augment as A
    B, H, W, s = 3, 24, 32, 32
    sv, sl = _pair(10, B, H, W)
    targets = batch_targets(B)
    random.seed(9)
    np.random.seed(9)
    Ms, rects, luts, flips, want_t, size = restated_batch(targets.numpy().astype(np.float64), B, H, W, s, BATCH_HYP, mosaic)
    want_v, want_l = R.augment(sv, sl, B, rects, (2 * s, 2 * s) if mosaic else None, np.stack([R.invert(m) for m in Ms]), size, luts, flips)
    random.seed(9)
    np.random.seed(9)
    ov, ol, got = A.augment_batch(_dev(sv), _dev(sl), targets, BATCH_HYP, mosaic=mosaic, img_size=s)
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    assert tuple(got.shape) == want_t.shape and np.allclose(got.numpy(), want_t, rtol=0, atol=1e-6)


def test_augment_batch_with_zero_affine_is_jitter_and_flip_only():
    from build_utils import augment as A
    B, H, W = 3, 20, 27
    sv, sl = _pair(11, B, H, W)
    hyp = dict(BATCH_HYP, degrees=0, translate=0, scale=0, shear=0)
    targets = batch_targets(B)
    random.seed(13)
    np.random.seed(13)
    _, _, luts, flips, want_t, _ = restated_batch(targets.numpy().astype(np.float64), B, H, W, max(H, W), hyp, False)
    want_v, want_l = R.augment(sv, sl, luts=luts, flip=flips)         # no matrix at all
    assert 0 < sum(flips) < B
    random.seed(13)
    np.random.seed(13)
    ov, ol, got = A.augment_batch(_dev(sv), _dev(sl), targets, hyp)
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    assert np.allclose(got.numpy(), want_t, rtol=0, atol=1e-6)
