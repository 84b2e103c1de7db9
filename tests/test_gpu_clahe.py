"""dyk_clahe and dyk_cutout_rects on the GPU (csrc/clahe.hip, dyk.functional.clahe / cutout, build_utils.snowflake) against the
plain numpy yardstick tests/clahe_ref.py: uint8 outputs and tables, so every comparison is bit for bit -- there is no tolerance
anywhere in this file.  Shapes and rules: tests/clahe_cases.py; what holds the yardstick itself to OpenCV's published
algorithm: tests/test_clahe_reference.py.  Nothing here is pinned against cv2: there is none to run."""
import ctypes

import numpy as np
import pytest
import torch

import clahe_cases as CC
import clahe_ref

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
    payload aligned for the vector paths; an odd lead takes the byte paths"""
    whole = torch.full((lead + nbytes + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[lead:lead + nbytes]


def _frame_intact(whole, lead):
    return bool((whole[:lead] == SENTINEL).all()) and bool((whole[-TAIL:] == SENTINEL).all())


def _run(imgs, clip_limit, grid, aligned=True, in_place=False):
    """dyk_clahe through the C ABI on framed buffers -> (rc, dst, tables, frames intact, src afterwards)"""
    L, h = _lib()
    P, H, W = imgs.shape
    leads = (256, 256, 256) if aligned else (3, 1, 5)
    ws = h.dyk_clahe_ws_bytes(P, grid[0], grid[1])
    src_w, src = _framed(imgs.size, leads[0])
    src.copy_(torch.from_numpy(np.array(imgs)).reshape(-1))
    dst_w, dst = (src_w, src) if in_place else _framed(imgs.size, leads[1])
    lut_w, lut = _framed(ws, leads[2])
    d = L.DykClaheDesc(src=src.data_ptr(), dst=dst.data_ptr(), lut=lut.data_ptr(), planes=P, H=H, W=W, tiles_x=grid[0],
                       tiles_y=grid[1], clip_limit=clip_limit)
    rc = h.dyk_clahe(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    intact = _frame_intact(src_w, leads[0]) and _frame_intact(dst_w, leads[0] if in_place else leads[1]) and _frame_intact(lut_w, leads[2])
    return (rc, dst.cpu().numpy().reshape(imgs.shape), lut.cpu().numpy().reshape(P, grid[0] * grid[1], 256), intact,
            src.cpu().numpy().reshape(imgs.shape))


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd_bases"])
@pytest.mark.parametrize("name", CC.SMALL)
def test_output_and_tables_equal_the_yardstick_bit_for_bit(name, aligned):
    c = CC.case(name)
    want_dst, want_lut = CC.reference(name)
    rc, dst, lut, intact, src = _run(c["imgs"], c["clip_limit"], c["grid"], aligned)
    assert rc == 0
    assert np.array_equal(lut, want_lut), "tables differ in %d entries" % int((lut != want_lut).sum())
    assert np.array_equal(dst, want_dst), "output differs in %d pixels" % int((dst != want_dst).sum())
    assert intact and np.array_equal(src, c["imgs"])


def test_full_size_plane_twice_and_in_place():
    """512 x 640 at the reference's (4, 4): 160 x 128 tiles.  Two runs give the same bytes, and so does dst == src."""
    name = "full_512x640"
    c = CC.case(name)
    want_dst, want_lut = CC.reference(name)
    rc, dst, lut, intact, _ = _run(c["imgs"], c["clip_limit"], c["grid"])
    assert rc == 0 and intact
    assert np.array_equal(lut, want_lut) and np.array_equal(dst, want_dst)
    rc2, dst2, lut2, intact2, _ = _run(c["imgs"], c["clip_limit"], c["grid"])
    assert rc2 == 0 and intact2 and np.array_equal(dst2, dst) and np.array_equal(lut2, lut)
    rc3, dst3, lut3, intact3, _ = _run(c["imgs"], c["clip_limit"], c["grid"], in_place=True)
    assert rc3 == 0 and intact3 and np.array_equal(dst3, dst) and np.array_equal(lut3, lut)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd_bases"])
@pytest.mark.parametrize("name", ["10x13_g4", "33x47_g16x3", "noise_96x97", "clip2", "planes7", "planes7_words"])
def test_in_place_and_repeated_runs_give_the_same_bytes(name, aligned):
    c = CC.case(name)
    want_dst, want_lut = CC.reference(name)
    for _ in range(2):
        rc, dst, lut, intact, _src = _run(c["imgs"], c["clip_limit"], c["grid"], aligned, in_place=True)
        assert rc == 0 and intact
        assert np.array_equal(dst, want_dst) and np.array_equal(lut, want_lut)


def test_refused_arguments_return_err_arg_and_write_nothing():
    L, h = _lib()
    for H, W, grid in CC.REFUSED:
        n = max(H, 1) * max(W, 1)
        src_w, src = _framed(n, 256)
        dst_w, dst = _framed(n, 256)
        lut_w, lut = _framed(max(grid[0], 1) * max(grid[1], 1) * 256, 256)
        d = L.DykClaheDesc(src=src.data_ptr(), dst=dst.data_ptr(), lut=lut.data_ptr(), planes=1, H=H, W=W, tiles_x=grid[0],
                           tiles_y=grid[1], clip_limit=1.0)
        assert h.dyk_clahe(ctypes.byref(d), _stream()) == -1, (H, W, grid)
        torch.cuda.synchronize()
        for t in (src_w, dst_w, lut_w):
            assert bool((t == SENTINEL).all()), (H, W, grid)
    src_w, src = _framed(64, 256)
    lut_w, lut = _framed(1024, 256)
    for kw in ({"src": None}, {"dst": None}, {"lut": None}, {"planes": 0}):
        args = dict(src=src.data_ptr(), dst=src.data_ptr(), lut=lut.data_ptr(), planes=1, H=8, W=8, tiles_x=2, tiles_y=2, clip_limit=1.0)
        args.update(kw)
        assert h.dyk_clahe(ctypes.byref(L.DykClaheDesc(**args)), _stream()) == -1, kw
    assert h.dyk_clahe(None, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((src_w == SENTINEL).all()) and bool((lut_w == SENTINEL).all())


def test_functional_clahe_refuses_what_the_rule_refuses():
    from dyk import functional as F
    for H, W, grid in CC.REFUSED:
        with pytest.raises(ValueError):
            F.clahe(torch.zeros((1, H, W), dtype=torch.uint8, device="cuda"), 1.0, grid)
    img = torch.zeros((3, 8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        F.clahe(img.float())
    with pytest.raises(TypeError):
        F.clahe(img.cpu())
    with pytest.raises(TypeError):
        F.clahe(img, 1.0, 4)
    with pytest.raises(ValueError):
        F.clahe(img.permute(1, 2, 0))                                 # interleaved view: not contiguous
    with pytest.raises(ValueError):
        F.clahe(img, out=torch.zeros((3, 8, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        F.cutout(img, torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        F.cutout(img, torch.zeros((2, 1, 4), dtype=torch.int32))      # two sets for three planes of one image
    with pytest.raises(ValueError):
        F.cutout(img, torch.zeros((1, 4), dtype=torch.int32), value=256)


def test_functional_clahe_on_a_loader_batch():
    """[B,3,H,W] as the loader emits it, default arguments = the reference's clipLimit 1.0 and 4 x 4 grid; out= and in place"""
    from dyk import functional as F
    imgs = np.concatenate([CC.noise("batch", 3, 24, 36), CC.peaked("batch", 3, 24, 36)]).reshape(2, 3, 24, 36)
    want = clahe_ref.clahe(imgs, 1.0, (4, 4))[0]
    x = torch.from_numpy(imgs).cuda()
    y = F.clahe(x)
    assert y.dtype == torch.uint8 and y.shape == x.shape and y.data_ptr() != x.data_ptr()
    assert np.array_equal(y.cpu().numpy(), want) and np.array_equal(x.cpu().numpy(), imgs)
    out = torch.empty_like(x)
    assert F.clahe(x, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert F.clahe(x, out=x) is x and np.array_equal(x.cpu().numpy(), want)
    want2 = clahe_ref.clahe(imgs[0, 0], 2.5, (3, 2))[0]
    assert np.array_equal(F.clahe(torch.from_numpy(imgs[0, 0]).cuda(), 2.5, (3, 2)).cpu().numpy(), want2)


# ---------------------------------------------------------------------------------------------- cut-outs
@pytest.mark.parametrize("lead", [256, 3], ids=["aligned", "odd_base"])
@pytest.mark.parametrize("name", list(CC.CUT_CASES))
def test_cutout_rects_equals_numpy_slicing(name, lead):
    L, h = _lib()
    c = CC.cut_case(name)
    P, H, W = c["imgs"].shape
    want = clahe_ref.cutout(c["imgs"], c["rects"], c["planes_per_set"], c["value"])
    whole, img = _framed(c["imgs"].size, lead)
    img.copy_(torch.from_numpy(np.array(c["imgs"])).reshape(-1))
    rects = torch.from_numpy(np.array(c["rects"])).cuda()
    rc = h.dyk_cutout_rects(img.data_ptr(), P, H, W, rects.data_ptr(), c["rects"].shape[1], c["planes_per_set"], c["value"], _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _frame_intact(whole, lead)
    assert np.array_equal(img.cpu().numpy().reshape(P, H, W), want)
    assert np.array_equal(rects.cpu().numpy(), c["rects"])


def test_cutout_refused_arguments_write_nothing():
    L, h = _lib()
    whole, img = _framed(3 * 8 * 8, 256)
    rects = torch.tensor([[[0, 0, 8, 8]]], dtype=torch.int32, device="cuda")
    ok = dict(img=img.data_ptr(), planes=3, H=8, W=8, rects=rects.data_ptr(), nrect=1, pps=3, value=0)
    for kw in ({"img": None}, {"planes": 0}, {"H": 0}, {"W": -1}, {"rects": None}, {"nrect": -1}, {"pps": 0}, {"value": 256}, {"value": -1}):
        a = dict(ok, **kw)
        assert h.dyk_cutout_rects(a["img"], a["planes"], a["H"], a["W"], a["rects"], a["nrect"], a["pps"], a["value"], _stream()) == -1, kw
    assert h.dyk_cutout_rects(ok["img"], 3, 8, 8, None, 0, 3, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((whole == SENTINEL).all())


def test_functional_cutout_takes_host_and_device_rectangles():
    from dyk import functional as F
    c = CC.cut_case("two_sets")
    imgs = c["imgs"].reshape(2, 3, 20, 30)
    want = clahe_ref.cutout(c["imgs"], c["rects"], 3, 0).reshape(imgs.shape)
    for rects in (torch.from_numpy(np.array(c["rects"])), torch.from_numpy(np.array(c["rects"])).cuda()):
        x = torch.from_numpy(np.array(imgs)).cuda()
        assert F.cutout(x, rects) is x
        assert np.array_equal(x.cpu().numpy(), want)
    # [nrect, 4]: one set for every plane; a value other than 0; no rectangles at all
    one = c["rects"][0]
    x = torch.from_numpy(np.array(imgs)).cuda()
    F.cutout(x, torch.from_numpy(np.array(one)), value=9)
    assert np.array_equal(x.cpu().numpy().reshape(6, 20, 30), clahe_ref.cutout(c["imgs"], one[None], 6, 9))
    y = torch.from_numpy(np.array(imgs)).cuda()
    F.cutout(y, torch.zeros((0, 4), dtype=torch.int32))
    assert np.array_equal(y.cpu().numpy(), imgs)


# ---------------------------------------------------------------------------------------------- build_utils.snowflake
def _expected_pair(v, l, labels, rand, xywh=True, clahe=True, label_thr=0.35, n_thr=6, step=16, n_snow=25, clip_limit=1.0,
                   grid=(4, 4)):
    """the composition the module must equal, restated with loops: yardstick CLAHE, the reference's boxes from `rand`
    (a RandomState at the state np.random is in), the label filter, numpy slicing.  -> (v, l, keep mask, margin of the
    closest keep decision)"""
    if clahe:
        v, l = clahe_ref.clahe(v, clip_limit, grid)[0], clahe_ref.clahe(l, clip_limit, grid)[0]
    v, l = np.array(v, copy=True), np.array(l, copy=True)
    keep, margin = np.ones(len(labels), bool), np.inf
    if len(labels) <= n_thr:
        rows, cols = v.shape[1], v.shape[2]
        boxes = []
        for a, b in rand.rand(n_snow, 2):
            x, y = a * (rows - 1), b * (cols - 1)                 # the reference draws x over the rows and y over the columns
            boxes.append([np.floor(x), np.floor(y), np.floor(min(x + step - 1, rows - 1)), np.floor(min(y + step - 1, cols - 1))])
        for i, lab in enumerate(labels):
            if xywh:
                xc, yc, w, h = (np.float32(t) for t in lab[1:5])
                x1, y1, x2, y2 = (xc - w / 2) * rows, (yc - h / 2) * cols, (xc + w / 2) * rows, (yc + h / 2) * cols
            else:
                x1, y1, x2, y2 = lab[1:5]
            area = max(float((x2 - x1) * (y2 - y1)), 1.0)
            total = 0.0
            for bx1, by1, bx2, by2 in boxes:
                sx = min(max(min(float(x2), bx2) - max(float(x1), bx1), 0.0), float(n_snow))
                sy = min(max(min(float(y2), by2) - max(float(y1), by1), 0.0), float(n_snow))
                total += sx * sy / area
            keep[i] = total < label_thr
            margin = min(margin, abs(total - label_thr))
        for bx1, by1, bx2, by2 in boxes:
            v[:, int(by1):int(by2), int(bx1):int(bx2)] = 0
            l[:, int(by1):int(by2), int(bx1):int(bx2)] = 0
    return v, l, keep, margin


def _pair(name, H=48, W=72):
    return CC.noise(name + "v", 3, H, W), CC.peaked(name + "l", 3, H, W)


LABELS = np.array([[0, 0.30, 0.40, 0.50, 0.60], [0, 0.70, 0.55, 0.10, 0.12], [1, 0.20, 0.80, 0.08, 0.30], [0, 0.55, 0.25, 0.30, 0.25]],
                  np.float32)


def test_clahe_image_is_the_yardstick_on_both_streams():
    from build_utils.snowflake import clahe_image
    v, l = _pair("ci")
    gv, gl = clahe_image(torch.from_numpy(v).cuda(), torch.from_numpy(l).cuda())
    assert np.array_equal(gv.cpu().numpy(), clahe_ref.clahe(v)[0]) and np.array_equal(gl.cpu().numpy(), clahe_ref.clahe(l)[0])
    bv, bl = np.stack([v, l]), np.stack([l, v])
    gv, gl = clahe_image(torch.from_numpy(bv).cuda(), torch.from_numpy(bl).cuda(), 2.0, (3, 5))
    assert np.array_equal(gv.cpu().numpy(), clahe_ref.clahe(bv, 2.0, (3, 5))[0])
    assert np.array_equal(gl.cpu().numpy(), clahe_ref.clahe(bl, 2.0, (3, 5))[0])


@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy_labels", "tensor_labels"])
def test_snowflake_cutout_equals_the_composition(as_tensor):
    from build_utils.snowflake import snowflake_cutout
    v, l = _pair("sc")
    seed = 14
    wv, wl, keep, margin = _expected_pair(v, l, LABELS, np.random.RandomState(seed))
    assert margin > 1e-6 and keep.any() and not keep.all()        # one label dropped, one kept, none on the edge
    np.random.seed(seed)
    labels = torch.from_numpy(LABELS.copy()) if as_tensor else LABELS.copy()
    tv, tl = torch.from_numpy(v).cuda(), torch.from_numpy(l).cuda()
    gv, gl, gl_labels = snowflake_cutout(tv, tl, labels)
    assert np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(gl.cpu().numpy(), wl)
    assert isinstance(gl_labels, type(labels)) and np.array_equal(np.asarray(gl_labels), LABELS[keep])
    assert np.array_equal(tv.cpu().numpy(), v) and np.array_equal(tl.cpu().numpy(), l)        # with clahe the inputs stay
    assert (wv == 0).sum() > (clahe_ref.clahe(v)[0] == 0).sum()                                # and something was cut


def test_snowflake_cutout_without_clahe_with_pixel_labels_and_above_n_thr():
    from build_utils.snowflake import snowflake_cutout
    v, l = _pair("sp")
    rows, cols = v.shape[1:]
    pix = np.array([[0, 5, 9, 30, 40], [1, 20, 30, 26, 37], [0, 1, 1, 47, 70]], np.float32)         # class, xyxy in pixels
    kw = dict(xywh=False, clahe=False, label_thr=0.2, step=8, n_snow=12)
    wv, wl, keep, margin = _expected_pair(v, l, pix, np.random.RandomState(5), **kw)
    assert margin > 1e-6
    np.random.seed(5)
    tv, tl = torch.from_numpy(v).cuda(), torch.from_numpy(l).cuda()
    gv, gl, got = snowflake_cutout(tv, tl, pix.copy(), **kw)
    assert gv is tv and gl is tl                                  # without clahe the cut-outs go into the images given
    assert np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(gl.cpu().numpy(), wl) and np.array_equal(got, pix[keep])
    # more labels than n_thr: CLAHE only, every label kept, no random number drawn
    many = np.tile(LABELS, (2, 1))
    np.random.seed(5)
    gv, gl, got = snowflake_cutout(torch.from_numpy(v).cuda(), torch.from_numpy(l).cuda(), many)
    assert np.array_equal(gv.cpu().numpy(), clahe_ref.clahe(v)[0]) and np.array_equal(gl.cpu().numpy(), clahe_ref.clahe(l)[0])
    assert np.array_equal(got, many) and np.random.rand() == np.random.RandomState(5).rand()


def test_snowflake_batch_equals_the_composition_per_image():
    """three images: four labels (one dropped), eight labels (above n_thr: uncut, all kept), none (cut all the same); the
    targets come interleaved, as no collate function emits them, to show that the row order is kept"""
    from build_utils.snowflake import snowflake_batch
    pairs = [_pair("b%d" % i) for i in range(3)]
    per_image = [LABELS, np.tile(LABELS, (2, 1)), LABELS[:0]]
    rows = [np.concatenate([[b], lab]) for b, labs in enumerate(per_image) for lab in labs]
    order = np.random.RandomState(1).permutation(len(rows))
    targets = np.array(rows, np.float32)[order]
    seed = 14
    rand = np.random.RandomState(seed)
    want_v, want_l, keep = [], [], np.ones(len(targets), bool)
    for b, (v, l) in enumerate(pairs):
        mine = np.nonzero(targets[:, 0] == b)[0]
        wv, wl, k, margin = _expected_pair(v, l, targets[mine, 1:], rand)
        assert margin > 1e-6
        want_v.append(wv)
        want_l.append(wl)
        keep[mine] = k
    assert not keep.all() and keep[targets[:, 0] == 1].all()
    assert np.array_equal(want_v[1], clahe_ref.clahe(pairs[1][0])[0])                           # the crowded image stays uncut
    np.random.seed(seed)
    bv = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    bl = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    for tg in (targets.copy(), torch.from_numpy(targets.copy())):
        np.random.seed(seed)
        gv, gl, got = snowflake_batch(bv, bl, tg)
        assert np.array_equal(gv.cpu().numpy(), np.stack(want_v)) and np.array_equal(gl.cpu().numpy(), np.stack(want_l))
        assert isinstance(got, type(tg)) and np.array_equal(np.asarray(got), targets[keep])


# ---------------------------------------------------------------------------------------------- wrong kernels (CPU side)
@pytest.mark.parametrize("mutant", sorted(CC.WITNESS))
def test_a_wrong_kernel_would_be_flagged(mutant):
    """each plausible mistake of a CLAHE / cut-out kernel, made in the yardstick, changes the bytes of a named case of the
    matrix above: a kernel that made it would fail test_output_and_tables_equal_the_yardstick_bit_for_bit on that case"""
    assert CC.WITNESS[mutant] in CC.CASES or CC.WITNESS[mutant] in CC.CUT_CASES
    assert CC.flagged(mutant)
