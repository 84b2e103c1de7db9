"""dyk_resize_pad_pairs on the GPU (csrc/letterbox.hip, dyk.functional.resize_pad_pairs, build_utils.letterbox) against the plain
numpy yardstick tests/letterbox_ref.py: uint8 outputs, so every image comparison is bit for bit -- there is no tolerance on
pixels anywhere in this file.  Shapes and rules: tests/letterbox_cases.py; what holds the yardstick itself:
tests/test_letterbox_reference.py.  Nothing here is pinned against cv2: there is none to run."""
import ctypes

import numpy as np
import pytest
import torch

import letterbox_cases as LC
import letterbox_ref as R

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
    payload aligned for the wide loads and dword stores; an odd lead takes the byte paths"""
    whole = torch.full((lead + nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[lead:lead + nbytes]


def _frame_intact(whole, lead):
    return bool((whole[:lead] == SENTINEL).all()) and bool((whole[-TAIL:] == SENTINEL).all())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the cases are read-only)


def _run(name, aligned=True):
    """the case through the C ABI on framed buffers -> (rc, dst_v, dst_l, frames intact, sources unchanged)"""
    L, h = _lib()
    c = LC.case(name)
    B = len(c["geom"])
    Ho, Wo = c["out_size"]
    odd = (3, 1, 5, 7, 9, 11, 13, 15)
    srcs, frames = [[], []], []
    for s, imgs in enumerate((c["v"], c["l"])):
        for b, a in enumerate(imgs):
            lead = 256 if aligned else odd[(2 * b + s) % 8]
            w, p = _framed(a.size, lead)
            p.copy_(torch.from_numpy(np.array(a)).reshape(-1))
            srcs[s].append(p)
            frames.append((w, lead))
    dsts = []
    for k in range(2):
        lead = 256 if aligned else (5, 7)[k]
        w, p = _framed(B * 3 * Ho * Wo, lead)
        dsts.append(p)
        frames.append((w, lead))
    recs = (L.DykResizePadRec * B)()
    for b in range(B):
        a = c["v"][b]
        hh, ww = a.shape[1:] if c["layout"] == "chw" else a.shape[:2]
        nh, nw, top, left, interp = c["geom"][b]
        recs[b] = L.DykResizePadRec(src_v=srcs[0][b].data_ptr(), src_l=srcs[1][b].data_ptr(), h=hh, w=ww, nh=nh, nw=nw, top=top, left=left,
                                    interp=interp)
    drecs = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).cuda()
    d = L.DykResizePadDesc(recs=drecs.data_ptr(), recs_host=ctypes.addressof(recs), dst_v=dsts[0].data_ptr(), dst_l=dsts[1].data_ptr(), B=B,
                           Ho=Ho, Wo=Wo, layout={"chw": 0, "hwc_bgr": 1}[c["layout"]], color=(ctypes.c_uint8 * 3)(*c["color"]))
    rc = h.dyk_resize_pad_pairs(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    intact = all(_frame_intact(w, lead) for w, lead in frames)
    same = all(np.array_equal(p.cpu().numpy().reshape(a.shape), a) for s, imgs in enumerate((c["v"], c["l"])) for p, a in zip(srcs[s], imgs))
    shape = (B, 3, Ho, Wo)
    return rc, dsts[0].cpu().numpy().reshape(shape), dsts[1].cpu().numpy().reshape(shape), intact, same


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s differs in %d of %d bytes" % (what, int((got != want).sum()), want.size)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd_bases"])
@pytest.mark.parametrize("name", LC.SMALL)
def test_both_outputs_equal_the_yardstick_bit_for_bit(name, aligned):
    want_v, want_l = LC.reference(name)
    rc, ov, ol, intact, same = _run(name, aligned)
    assert rc == 0
    _equal(ov, want_v, "visible")
    _equal(ol, want_l, "lwir")
    assert intact and same


def test_full_size_batch_twice():
    """16 pairs of 512 x 640 -> 410 x 512 content in 512 x 512, LINEAR and AREA alternating: equal to the yardstick, and two runs
    give the same bytes"""
    want_v, want_l = LC.reference(LC.FULL)
    rc, ov, ol, intact, same = _run(LC.FULL)
    assert rc == 0 and intact and same
    _equal(ov, want_v, "visible")
    _equal(ol, want_l, "lwir")
    rc2, ov2, ol2, intact2, _ = _run(LC.FULL)
    assert rc2 == 0 and intact2 and np.array_equal(ov2, ov) and np.array_equal(ol2, ol)


@pytest.mark.parametrize("name", ["up_9x13", "area_w37", "hwc_batch3_mixed", "unstaged_area", "steep_area_64"])
def test_two_runs_give_identical_bytes(name):
    a, b = _run(name), _run(name, aligned=False)
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", LC.SMALL)
def test_functional_resize_pad_pairs_equals_the_yardstick(name):
    from dyk import functional as F
    c = LC.case(name)
    want_v, want_l = LC.reference(name)
    v, l = [_dev(a) for a in c["v"]], [_dev(a) for a in c["l"]]
    if len(v) == 1:                                               # one image: the batch-tensor form
        v, l = v[0][None], l[0][None]
    ov, ol = F.resize_pad_pairs(v, l, c["geom"], c["out_size"], layout=c["layout"], color=c["color"])
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")


def test_functional_resize_pad_pairs_refuses_what_the_rule_refuses():
    from dyk import functional as F
    v = torch.zeros((2, 3, 8, 12), dtype=torch.uint8, device="cuda")
    l = torch.zeros_like(v)
    ok = [(4, 6, 0, 0, 0)] * 2
    out = (torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda"), torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device="cuda"))
    F.resize_pad_pairs(v, l, ok, (8, 8), out=out)                 # the admitted call
    for geom in ([(9, 6, 0, 0, 1)] * 2, [(4, 13, 0, 0, 1)] * 2, [(4, 6, 5, 0, 0)] * 2, [(4, 6, 0, 3, 0)] * 2, [(4, 6, -1, 0, 0)] * 2,
                 [(0, 6, 0, 0, 0)] * 2, [(4, 6, 0, 0, 2)] * 2, ok[:1]):
        with pytest.raises(ValueError):
            F.resize_pad_pairs(v, l, geom, (8, 8))
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 16385))
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 8), layout="hwc")
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 8), layout="hwc_bgr")    # [3,8,12] is no [h,w,3]
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 8), color=(0, 0, 256))
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l[:, :, :4], ok, (8, 8))            # the streams differ in size
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v.permute(0, 1, 3, 2), l.permute(0, 1, 3, 2), ok, (8, 8))
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 8), out=(out[0], out[0]))           # the outputs overlap
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, [(8, 12, 0, 0, 0)] * 2, (8, 12), out=(v, l))  # an output over its input
    with pytest.raises(ValueError):
        F.resize_pad_pairs(v, l, ok, (8, 8), out=(out[0][:, :, :4], out[1][:, :, :4]))
    with pytest.raises(TypeError):
        F.resize_pad_pairs(v.float(), l.float(), ok, (8, 8))
    with pytest.raises(TypeError):
        F.resize_pad_pairs(v.cpu(), l.cpu(), ok, (8, 8))
    with pytest.raises(TypeError):
        F.resize_pad_pairs([np.zeros((3, 8, 12), np.uint8)] * 2, [np.zeros((3, 8, 12), np.uint8)] * 2, ok, (8, 8))
    with pytest.raises(TypeError):
        F.resize_pad_pairs(v, l, ok, (8, 8), out=(out[0].float(), out[1].float()))
    assert not v.any() and not l.any()


# ---------------------------------------------------------------------------------------------- build_utils.letterbox
def _pair(seed, h, w, layout="chw"):
    r = np.random.RandomState(seed)
    shape = (3, h, w) if layout == "chw" else (h, w, 3)
    return r.randint(0, 256, shape).astype(np.uint8), r.randint(0, 256, shape).astype(np.uint8)


def _ref_letterbox(imgs, new_shape, color=(0, 0, 0), interp=R.LINEAR, **kw):
    """the yardstick composed on the host: planar images of one size -> (outputs, ratio, pad)"""
    ratio, pad, (nh, nw), (top, bottom, left, right) = R.letterbox_geometry(imgs[0].shape[1:], new_shape, **kw)
    ov, ol = R.resize_pad([imgs[0]], [imgs[1]], [(nh, nw, top, left, interp)], (nh + top + bottom, nw + left + right), color=color)
    return (ov[0], ol[0]), ratio, pad


@pytest.mark.parametrize("shape,new_shape,kw", [((40, 50), 32, dict(auto=True)), ((40, 50), 32, dict(auto=False)),
                                                ((20, 30), (64, 96), dict(auto=False, scale_up=False)),
                                                ((20, 30), (64, 96), dict(auto=False, scale_up=True)),
                                                ((10, 20), (32, 48), dict(auto=False, scale_fill=True)),
                                                ((41, 53), (416, 416), dict())],
                         ids=["auto", "plain", "no_scale_up", "scale_up", "scale_fill", "defaults"])
def test_letterbox_and_letterbox_pair(shape, new_shape, kw):
    from build_utils import letterbox as LB
    sv, sl = _pair(1, *shape)
    (want_v, want_l), ratio, pad = _ref_letterbox((sv, sl), new_shape, color=(114, 114, 114), **kw)
    ov, ol, r2, p2 = LB.letterbox_pair(_dev(sv), _dev(sl), new_shape, color=(114, 114, 114), **kw)
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    assert tuple(r2) == ratio and tuple(float(t) for t in p2) == pad
    img, r1, p1 = LB.letterbox(_dev(sl), new_shape, color=(114, 114, 114), **kw)
    _equal(img.cpu().numpy(), want_l, "single image")
    assert tuple(r1) == ratio and tuple(float(t) for t in p1) == pad


def test_load_resize():
    from build_utils import letterbox as LB
    sv, sl = _pair(2, 32, 40)
    for img_size, augment, size, interp in [(32, False, (25, 32), R.AREA), (32, True, (25, 32), R.LINEAR), (50, False, (40, 50), R.LINEAR)]:
        want = R.resize_pad([sv], [sl], [size + (0, 0, interp)], size)
        ov, ol, s0, s1 = LB.load_resize(_dev(sv), _dev(sl), img_size, augment)
        _equal(ov.cpu().numpy(), want[0][0], "visible")
        _equal(ol.cpu().numpy(), want[1][0], "lwir")
        assert s0 == (32, 40) and s1 == size
    v, l = _dev(sv), _dev(sl)
    ov, ol, s0, s1 = LB.load_resize(v, l, 40, False)
    assert ov is v and ol is l and s0 == s1 == (32, 40)           # r == 1: untouched


def _ref_batch(vs, ls, new_shape, img_size, augment, layout, color=(0, 0, 0)):
    """load_normal_images per sample with the yardstick: two successive resizes where the reference makes two"""
    outs, shapes = [[], []], []
    for v, l in zip(vs, ls):
        pv, pl = R.planes_of(v, layout), R.planes_of(l, layout)
        h0, w0 = pv.shape[1:]
        h, w = h0, w0
        if img_size is not None:
            r = img_size / max(h0, w0)
            if r != 1:
                h, w = int(h0 * r), int(w0 * r)
                interp = R.AREA if r < 1 and not augment else R.LINEAR
                a, b = R.resize_pad([pv], [pl], [(h, w, 0, 0, interp)], (h, w))
                pv, pl = a[0], b[0]
        (ov, ol), ratio, pad = _ref_letterbox((pv, pl), new_shape, color=color, auto=False, scale_up=augment)
        outs[0].append(ov)
        outs[1].append(ol)
        shapes.append(((h0, w0), ((h / h0, w / w0), pad)))
    return np.stack(outs[0]), np.stack(outs[1]), shapes


@pytest.mark.parametrize("form", ["tensor", "list", "hwc_bgr"])
def test_letterbox_batch_in_one_launch(form, monkeypatch):
    from build_utils import letterbox as LB
    from dyk import functional as F
    layout = "hwc_bgr" if form == "hwc_bgr" else "chw"
    sizes = [(32, 40)] * 3 if form == "tensor" else [(32, 40), (40, 32), (20, 40)]
    pairs = [_pair(10 + i, h, w, layout) for i, (h, w) in enumerate(sizes)]
    vs, ls = [p[0] for p in pairs], [p[1] for p in pairs]
    want_v, want_l, want_shapes = _ref_batch(vs, ls, 32, 32, False, layout, color=(114, 114, 114))
    calls = []
    real = F.resize_pad_pairs
    monkeypatch.setattr(F, "resize_pad_pairs", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    dv, dl = [_dev(a) for a in vs], [_dev(a) for a in ls]
    if form == "tensor":
        dv, dl = torch.stack(dv), torch.stack(dl)
    labels = [np.array([[0, 0.5, 0.5, 0.2, 0.4], [1, 0.25, 0.75, 0.1, 0.1]]), np.zeros((0, 5)), np.array([[0, 0.3, 0.6, 0.2, 0.2]])]
    ov, ol, shapes, labs = LB.letterbox_batch(dv, dl, 32, img_size=32, augment=False, color=(114, 114, 114), layout=layout, labels=labels)
    assert len(calls) == 1                                        # the load_image resize only; the letterbox only pads
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    assert shapes == want_shapes
    for x, got, ((h0, w0), ((rh, rw), pad)) in zip(labels, labs, shapes):
        h, w = int(h0 * 32 / max(h0, w0)), int(w0 * 32 / max(h0, w0))
        want = x.copy()
        if len(x):
            want[:, 1], want[:, 3] = w * (x[:, 1] - x[:, 3] / 2) + pad[0], w * (x[:, 1] + x[:, 3] / 2) + pad[0]
            want[:, 2], want[:, 4] = h * (x[:, 2] - x[:, 4] / 2) + pad[1], h * (x[:, 2] + x[:, 4] / 2) + pad[1]
        assert got.shape == want.shape and np.allclose(got, want, rtol=0, atol=1e-12)


def test_letterbox_batch_with_two_resizes_takes_two_launches(monkeypatch):
    """img_size 24 shrinks 32 x 40 to 19 x 24 (AREA), and new_shape 48 with augment's scale_up enlarges that to 38 x 48
    (LINEAR): the reference resizes twice, and so does the batch, from an intermediate"""
    from build_utils import letterbox as LB
    from dyk import functional as F
    pairs = [_pair(20 + i, 32, 40, "hwc_bgr") for i in range(2)]
    vs, ls = [p[0] for p in pairs], [p[1] for p in pairs]
    want_v, want_l, want_shapes = _ref_batch(vs, ls, 48, 24, True, "hwc_bgr")
    assert want_v.shape == (2, 3, 48, 48)
    calls = []
    real = F.resize_pad_pairs
    monkeypatch.setattr(F, "resize_pad_pairs", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ov, ol, shapes, labs = LB.letterbox_batch([_dev(a) for a in vs], [_dev(a) for a in ls], 48, img_size=24, augment=True, layout="hwc_bgr")
    assert len(calls) == 2 and labs is None and shapes == want_shapes
    _equal(ov.cpu().numpy(), want_v, "visible")
    _equal(ol.cpu().numpy(), want_l, "lwir")
    with pytest.raises(ValueError):
        # under auto, 32 x 40 ends at 128 x 128 (102 rows + 26) and 16 x 40 at 64 x 128 (51 rows + 77 % 64): no one batch
        LB.letterbox_batch([_dev(vs[0]), _dev(vs[0][:16])], [_dev(ls[0]), _dev(ls[0][:16])], 128, auto=True, scale_up=True, layout="hwc_bgr")


def test_labels_round_trip_through_scale_coords():
    """boxes of the raw frame -> letterbox_labels -> scale_coords with the returned shapes land where they started"""
    from build_utils import letterbox as LB
    from build_utils.utils import scale_coords
    sv, sl = _pair(30, 48, 64)                                    # img_size 32: r = 0.5, 24 x 32 exactly, then 4 rows of padding each side
    rng = np.random.RandomState(31)
    xy = rng.uniform(0.2, 0.8, (5, 2))
    wh = rng.uniform(0.05, 0.3, (5, 2))
    x = np.concatenate([np.zeros((5, 1)), xy, wh], 1)
    ov, ol, shapes, labs = LB.letterbox_batch(_dev(sv)[None], _dev(sl)[None], 32, img_size=32, augment=False, labels=[x])
    assert tuple(ov.shape) == (1, 3, 32, 32) and shapes[0] == ((48, 64), ((0.5, 0.5), (0.0, 4.0)))
    start = np.stack([64 * (x[:, 1] - x[:, 3] / 2), 48 * (x[:, 2] - x[:, 4] / 2), 64 * (x[:, 1] + x[:, 3] / 2), 48 * (x[:, 2] + x[:, 4] / 2)], 1)
    boxes = torch.from_numpy(labs[0][:, 1:5]).float()
    back = scale_coords((32, 32), boxes, shapes[0][0], shapes[0][1]).numpy()
    assert np.allclose(back, start, rtol=0, atol=64 * 2.0 ** -22)              # a few fp32 roundings at magnitude 64
