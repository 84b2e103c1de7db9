"""oracle/stem.py, the fp64 reference of the stem convolution and its derived per-element bounds (no GPU), at the cases
tests/test_gpu_stem_elements.py runs on the GPU (tests/stem_cases.py):
  * the reference is torch.nn.functional.conv2d and its autograd in float64, to 1e-12 relative;
  * fp32 emulations of the kernels' arithmetic written in torch stay inside every bound on every small case (plain fp32 conv; the
    three-term weight split with sequential fp32 accumulation and * 1/255f; the fp32 weight gradient in two summation orders; the
    sum-then-scale weight gradient; the fused dz in fp32 with bf16 rounding) -- each prints `STEMEMU <what> <largest error / bound> <case>`;
  * the bounds are not vacuous: each of eleven wrong kernels is flagged by a named case;
  * the ambiguous share of every fused case is under 1 %."""
import functools

import pytest
import torch
import torch.nn.functional as F

import stem_cases as SC
from oracle import stem as O

SMALL = [(g.id, co, s, u8) for g in SC.GEOS for co in (16, 32) for s in (1, 2) for u8 in (True, False)]
FL255 = torch.tensor(1.0 / 255.0, dtype=torch.float32)


def _oihw(w):
    return w.view(-1, 3, 3, 3).permute(0, 3, 1, 2).contiguous()            # [co][ky][kx][c] -> OIHW


def _report(what, ratio, bad, case):
    print("STEMEMU %s %.5f %s" % (what, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s: %d elements outside their bound, largest error / bound %.3f" % (what, case, bad, ratio)


def _flagged(res, what, case):
    ratio, bad = res
    assert bad > 0, "%s is NOT flagged by case %s (largest error / bound %.3f)" % (what, case, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------- emulations
def conv32(p, img=None):
    return F.conv2d(p.imgf if img is None else img, _oihw(p.w), stride=p.stride, padding=1)


def split3(w):
    """w = hi + mid + lo, each with 8 significant bits (truncation), as stem_fwd_u8t_kernel splits it"""
    trunc = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = trunc(w)
    r1 = w - hi
    mid = trunc(r1)
    r2 = r1 - mid
    lo = trunc(r2)
    assert torch.equal(hi.double() + mid.double() + lo.double(), w.double())
    return hi, mid, lo


def split_conv32(p, img8=None):
    """the MFMA forward's arithmetic: integer pixel values times the three weight terms (exact products), accumulated one after the
    other in fp32, the sum scaled by the rounded 1/255"""
    P = O.patches((p.img8 if img8 is None else img8).float(), p.stride)
    terms = split3(p.w)
    acc = torch.zeros(P.shape[0], p.cout, P.shape[2], P.shape[3])
    for tc in range(27):
        for t in terms:
            acc = acc + P[:, tc:tc + 1] * t[:, tc].view(1, -1, 1, 1)
    return acc * FL255


def act32(name, t):
    """the activations as act_fwd evaluates them, in fp32"""
    if name == "mish":
        e = torch.exp(t.clamp(max=20.0))
        n = e * (e + 2.0)
        return t * (n * (1.0 / (n + 2.0)))
    if name == "hard-swish":
        return t * (t + 3.0).clamp(0.0, 6.0) * torch.tensor(1.0 / 6.0)
    return O.act64(name, t)


def check_forward(p, y32, label, case):
    """raw stores, statistics and every eval epilogue of an fp32 accumulator field y32 against the bounds"""
    r = p.ref
    for dt, dtype in SC.DTYPES.items():
        tgt, b = O.out_bound(r, dtype)
        _report("%s-fwd-%s" % (label, dt), *O.check(O.store(y32, dtype), tgt, b), case)
        for act in SC.ACTS:
            z32 = act32(act, y32 * p.scale.view(1, -1, 1, 1) + p.shift.view(1, -1, 1, 1))
            tgt, b = O.affine_bound(r, p.scale, p.shift, act, dtype)
            _report("%s-%s-%s" % (label, act, dt), *O.check(O.store(z32, dtype), tgt, b), case)
    b1, b2 = O.stats_bound(r)
    _report(label + "-s1", *O.check(y32.sum((0, 2, 3)), r.S1, b1), case)
    _report(label + "-s2", *O.check((y32 * y32).sum((0, 2, 3)), r.S2, b2), case)
    big = torch.full_like(p.scale, SC.F16_OVERFLOW_SCALE)
    tgt, b = O.affine_bound(r, big, p.shift, "linear", torch.float16)
    _report(label + "-saturating-f16", *O.check(O.store(y32 * big.view(1, -1, 1, 1) + p.shift.view(1, -1, 1, 1), torch.float16), tgt, b), case)


@pytest.mark.parametrize("geo_id,cout,stride", sorted({c[:3] for c in SMALL}))
def test_reference_is_conv2d_in_float64(geo_id, cout, stride):
    p = SC.fwd_problem(geo_id, cout, stride)
    r = p.ref
    x = p.imgf.double()
    w = _oihw(p.w.double()).requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=1)
    assert y.shape == r.y.shape and float((y.detach() - r.y).abs().max()) <= 1e-12 * float(r.y.abs().max())
    assert torch.allclose(r.A_y, F.conv2d(x, _oihw(p.w.double().abs()), stride=stride, padding=1), rtol=1e-12, atol=1e-12)
    q = SC.wgrad_problem(geo_id, cout, stride, False, "f32", "random")
    y.backward(q.dy.double())
    want = w.grad.permute(0, 2, 3, 1).reshape(cout, 27)
    assert float((q.dw - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((q.A_dw >= q.dw.abs() * (1 - 1e-12)).all())
    # the eval epilogue's argument spans both signs and exceeds 6 (relu6's and hard-swish's upper knee)
    t = r.y * p.scale.double().view(1, -1, 1, 1) + p.shift.double().view(1, -1, 1, 1)
    assert float(t.min()) < 0 and float(t.max()) > 6
    assert float((r.y.abs() * SC.F16_OVERFLOW_SCALE).max()) > O.F16_MAX, "the saturating fp16 case does not saturate"


@pytest.mark.parametrize("geo_id,cout,stride,u8", SMALL)
def test_fp32_forward_emulations_stay_inside_every_bound(geo_id, cout, stride, u8):
    p = SC.fwd_problem(geo_id, cout, stride)
    case = "%s c%d s%d %s" % (geo_id, cout, stride, SC.img_kind(u8))
    check_forward(p, conv32(p), "conv32", case)
    if u8:
        check_forward(p, split_conv32(p), "split3", case)


def planes32(p, Pint):
    """the sum-then-scale weight gradient: one fp32 plane per segment (integer pixel values: exact on the exact field), each scaled by
    the rounded 1/255, the planes then summed in fp32"""
    sidx = SC.seg_index(p.geo, p.stride)
    planes = []
    for s in range(int(sidx.max()) + 1):
        m = (sidx == s).unsqueeze(1).float()
        planes.append(torch.einsum("boyx,btyx->ot", p.dy * m, Pint) * FL255)
    return torch.stack(planes)


@pytest.mark.parametrize("geo_id,cout,stride,u8", SMALL)
def test_fp32_weight_gradient_emulations_stay_inside_every_bound(geo_id, cout, stride, u8):
    for dt in ("bf16", "f32"):
        for field in ("exact", "random"):
            p = SC.wgrad_problem(geo_id, cout, stride, u8, dt, field)
            if field == "random" and p.n > 2048:
                continue
            case = "%s c%d s%d %s %s %s" % (geo_id, cout, stride, SC.img_kind(u8), dt, field)
            P32 = p.P.float()                                             # fp32(p) / 255 in fp32, or the float image
            # order A: all pixels in one fp32 reduction.  order B: a sum per output row, the rows added one after the other
            a = torch.einsum("boyx,btyx->ot", p.dy, P32)
            rows = torch.einsum("boyx,btyx->byot", p.dy, P32).reshape(-1, cout, 27)
            b = torch.zeros(cout, 27)
            for row in rows:
                b = b + row
            tgt, bound = SC.wgrad_bound(p, sum_then_scale=False)
            _report("wgrad-orderA", *O.check(p.old + a, tgt, bound), case)
            _report("wgrad-orderB", *O.check(p.old + b, tgt, bound), case)
            if u8:
                c = planes32(p, O.patches(p.img.float(), stride)).sum(0)
                tgt, bound = SC.wgrad_bound(p, sum_then_scale=True)
                _report("wgrad-sum-then-scale", *O.check(p.old + c, tgt, bound), case)


def fused_dz32(p, red, swap=False):
    """the fused apply's dz as the kernel evaluates it: replicas folded in fp64, the means in fp32, rounded to bf16"""
    v = lambda t: t.view(1, -1, 1, 1)
    invn = torch.tensor(1.0 / p.n, dtype=torch.float32)
    m1, m2 = red[:, 0].sum(0).float() * invn, red[:, 1].sum(0).float() * invn
    if swap:
        m1 = m2
    xh = (p.yraw - v(p.mean)) * v(p.rstd)
    return (v(p.scale) * (p.da - v(m1) - xh * v(m2))).bfloat16().float()


def fused_dw32(p, dzb):
    return p.old_dw + torch.einsum("boyx,btyx->ot", dzb, O.patches(p.img8.float(), p.stride)) * FL255


@pytest.mark.parametrize("slots", SC.FUSED_SLOTS)
@pytest.mark.parametrize("geo_id,cout,stride", SC.FUSED)
def test_fused_apply_emulation_and_ambiguous_share(geo_id, cout, stride, slots):
    p = SC.fused_problem(geo_id, cout, stride)
    red = SC.fused_red(p, slots)
    f = SC.fused_ref(p, red)
    case = "%s c%d s%d slots %d" % (geo_id, cout, stride, slots)
    print("STEMEMU ambiguous-share %.5f %s" % (f.share, case))
    assert f.share <= O.AMBIGUOUS_SHARE, "ambiguous share %.4f of case %s" % (f.share, case)
    dzb = fused_dz32(p, red)
    assert int((dzb.double() != f.dzb).sum()) <= int(f.ambiguous.sum()) and bool(((dzb.double() != f.dzb) <= f.ambiguous).all()), \
        "an fp32 dz rounds away from the reference outside the ambiguous set"
    tgt, b = O.fused_dw_bound(f, p.P, p.n, p.old_dw)
    _report("fused-dw", *O.check(fused_dw32(p, dzb), tgt, b), case)
    for name, S, old in (("dbeta", f.S1, p.old_db), ("dgamma", f.S2, p.old_dg)):
        tgt, b = O.sum_bound(S, old)
        _report("fused-" + name, *O.check(old + S.float(), tgt, b), case)


# ---------------------------------------------------------------------------------------------------- wrong kernels
def _fwd_bad(p, y32, dtype):
    tgt, b = O.out_bound(p.ref, dtype)
    return O.check(O.store(y32, dtype), tgt, b)


def _stats_bad(p, y32):
    b1, b2 = O.stats_bound(p.ref)
    return O.check(y32.sum((0, 2, 3)), p.ref.S1, b1), O.check((y32 * y32).sum((0, 2, 3)), p.ref.S2, b2)


@pytest.mark.parametrize("geo_id,stride,what", [("3x128", 1, "right halo"), ("5x12", 2, "bottom halo"), ("9x47", 2, "right and bottom halo")])
def test_wrong_halo_replicated_instead_of_zero(geo_id, stride, what):
    p = SC.fwd_problem(geo_id, 32, stride)
    xp = F.pad(F.pad(p.imgf, (0, 1, 0, 1), mode="replicate"), (1, 0, 1, 0))
    wrong = F.conv2d(xp, _oihw(p.w), stride=stride)
    assert wrong.shape == p.ref.y.shape and not torch.equal(wrong, conv32(p))
    for dt in ("bf16", "f32"):
        _flagged(_fwd_bad(p, wrong, SC.DTYPES[dt]), "a replicated " + what, "%s c32 s%d %s" % (geo_id, stride, dt))


@pytest.mark.parametrize("geo_id", ["7x520", "6x256"])
def test_wrong_second_staged_word_reads_zeros(geo_id):
    """stride 2: word 64 of a parked row starts at image column 2 x_begin + 252; only pixels 126 / 127 of a full segment read it"""
    p = SC.fwd_problem(geo_id, 32, 2)
    Wo = SC.out_hw(p.geo, 2)[1]
    wrong = conv32(p).clone()
    for xb in range(0, Wo - SC.SEG + 1, SC.SEG):
        xz = p.imgf.clone()
        xz[..., 2 * xb + 252:] = 0
        wrong[..., xb + 126:xb + 128] = conv32(p, xz)[..., xb + 126:xb + 128]
    for dt in ("bf16", "f16"):
        ratio, bad = _fwd_bad(p, wrong, SC.DTYPES[dt])
        assert 0 < bad <= 2 * (Wo // SC.SEG) * p.geo.B * 32 * SC.out_hw(p.geo, 2)[0]
        _flagged((ratio, bad), "a second staged word of zeros", "%s c32 s2 %s" % (geo_id, dt))


@pytest.mark.parametrize("geo_id,stride", [("5x132", 1), ("6x300", 2)])
def test_wrong_dead_pixels_of_a_partial_tile_in_the_statistics(geo_id, stride):
    """the lanes of the last tile beyond Wo compute on the zero-extended row: the first of them still sees the last image column"""
    p = SC.fwd_problem(geo_id, 32, stride)
    Wo = SC.out_hw(p.geo, stride)[1]
    ext = F.pad(p.imgf, (0, (-Wo % 32) * stride))
    y_ext = conv32(p, ext)
    assert y_ext.shape[3] == Wo + (-Wo % 32) and torch.equal(y_ext[..., :Wo - 1], conv32(p)[..., :Wo - 1])
    (r1, bad1), (r2, bad2) = _stats_bad(p, y_ext)
    assert bad1 + bad2 > 0 and bad2 > 0, "dead pixels in the statistics are NOT flagged by case %s c32 s%d (%.3f, %.3f)" % (geo_id, stride, r1, r2)


@pytest.mark.parametrize("cout,stride", [(32, 1), (32, 2), (16, 2)])
def test_wrong_statistics_from_stored_values(cout, stride):
    p = SC.const_problem(cout, stride)
    for y32 in (conv32(p), split_conv32(p)):
        (r1, bad1), (r2, bad2) = _stats_bad(p, y32)
        assert bad1 == 0 and bad2 == 0 and max(r1, r2) <= 1.0
        (r1, bad1), (r2, bad2) = _stats_bad(p, y32.bfloat16().float())
        assert bad1 == cout and bad2 == cout and r1 > 10 and r2 > 10, "statistics of the stored bf16 values are NOT flagged by the constant field c%d s%d (%.3f, %.3f)" % (cout, stride, r1, r2)


def test_wrong_division_by_256():
    p = SC.fwd_problem("9x47", 32, 1)
    wrong = conv32(p, p.img8.float() / 256.0)
    for dt in ("bf16", "f32", "f16"):
        _flagged(_fwd_bad(p, wrong, SC.DTYPES[dt]), "/ 256 in place of / 255 (forward)", "9x47 c32 s1 " + dt)
    (r1, bad1), (r2, bad2) = _stats_bad(p, wrong)
    assert bad2 > 0, "/ 256 is NOT flagged by the statistics of case 9x47 c32 s1"
    q = SC.wgrad_problem("6x300", 32, 1, True, "bf16", "exact")
    got = q.old + planes32(q, O.patches(q.img.float(), 1)).sum(0) * (255.0 / 256.0)
    _flagged(O.check(got, *SC.wgrad_bound(q, True)), "/ 256 in place of / 255 (weight gradient)", "6x300 c32 s1 u8 bf16 exact")


def test_wrong_filter_map():
    """register r of half-wave g holds filter (r & 3) + 8 (r >> 2) + 4 g; a kernel that stores it as (r & 3) + 4 (r >> 2) + 16 g"""
    p = SC.fwd_problem("4x4", 32, 1)
    perm = torch.empty(32, dtype=torch.long)
    for g in range(2):
        for r in range(16):
            perm[(r & 3) + 4 * (r >> 2) + 16 * g] = (r & 3) + 8 * (r >> 2) + 4 * g
    assert sorted(perm.tolist()) == list(range(32)) and perm.tolist() != list(range(32))
    _flagged(_fwd_bad(p, split_conv32(p)[:, perm], torch.bfloat16), "a permuted filter map", "4x4 c32 s1 bf16")


@functools.lru_cache(maxsize=None)
def _big():
    """the large weight-gradient case with its fp64 patches (kept here, not in the shared cache)"""
    p = SC.wgrad_problem(SC.BIG_WGRAD.id, 32, 1, True, "bf16", "exact", False)
    return p, O.patches(O.image_values(p.img), 1)


def _drop(p, P, mask):
    """dw of a kernel that leaves out the pixels of `mask` [B, Ho, Wo]"""
    return p.old.double() + p.dw - torch.einsum("boyx,btyx->ot", p.dy.double() * mask.unsqueeze(1).double(), P)


@pytest.mark.parametrize("geo_id,stride,field", [("6x300", 1, "random"), ("6x300", 2, "exact"), ("7x520", 1, "exact")])
def test_wrong_weight_gradient_loses_one_pixel_per_segment(geo_id, stride, field):
    p = SC.wgrad_problem(geo_id, 32, stride, True, "bf16", field)
    Wo = SC.out_hw(p.geo, stride)[1]
    last = torch.zeros(p.geo.B, p.dy.shape[2], Wo, dtype=torch.bool)
    for xb in range(0, Wo, SC.SEG):
        last[..., min(Wo, xb + SC.SEG) - 1] = True
    _flagged(O.check(_drop(p, p.P, last), *SC.wgrad_bound(p, True)), "one pixel lost per segment", "%s c32 s%d u8 bf16 %s" % (geo_id, stride, field))
    one = torch.zeros_like(last)
    one[-1, -1, Wo // 2] = True
    if field == "exact" and float((p.dy[-1, :, -1, Wo // 2].abs().view(-1, 1) * p.P[-1, :, -1, Wo // 2].view(1, -1)).max()) > 0:
        _flagged(O.check(_drop(p, p.P, one), *SC.wgrad_bound(p, True)), "a single lost pixel", "%s c32 s%d u8 bf16 exact" % (geo_id, stride))


def test_wrong_kernels_on_the_two_segment_weight_gradient():
    """205x260x7: three segments per row (128, 128, 4), two per workgroup, 2153 planes"""
    p, P = _big()
    geo = p.geo
    spw, planes = SC.wgrad_planes(geo, 1)
    assert (spw, planes) == (2, 2153) and planes > 512 * 4
    case = "205x260x7 c32 s1 u8 bf16 exact"
    bound = SC.wgrad_bound(p, True)
    assert O.check(p.old.double() + p.dw, *bound)[1] == 0
    sidx = SC.seg_index(geo, 1)
    # a single pixel of value >= 1 under a non-zero gradient, lost
    one = torch.zeros_like(sidx, dtype=torch.bool)
    one[3, 100, 200] = True
    assert float((p.dy[3, :, 100, 200].abs().view(-1, 1) * P[3, :, 100, 200].view(1, -1)).max()) >= 1.0 / 255.0
    _flagged(O.check(_drop(p, P, one), *bound), "a single lost pixel at n = 373100", case)
    _flagged(O.check(_drop(p, P, sidx % spw == 1), *bound), "the second segment of a two-segment workgroup skipped", case)
    _flagged(O.check(_drop(p, P, sidx // spw >= 512), *bound), "planes beyond 512 not folded", case)
    # stale dy in pixels [npx, roundup16(npx)): the 4-pixel segment 3 r + 2 follows a full one in its workgroup when it is odd (r odd);
    # pixels 4 .. 15 then keep the gradients of pixels 132 .. 143 of the row, and dead pixel 260 still sees image column 259 at kx = 0
    Ho = geo.H
    rows = torch.arange(geo.B * Ho).view(geo.B, Ho)
    stale = ((3 * rows + 2) % spw == 1).double()
    xp = F.pad(O.image_values(p.img), (1, 1, 1, 1))
    delta = torch.zeros(32, 27, dtype=torch.float64)
    for ky in range(3):
        for c in range(3):
            v = xp[:, c, ky:ky + Ho, 260] * stale                          # column 259 of the image, rows yo - 1 + ky
            delta[:, (ky * 3 + 0) * 3 + c] = torch.einsum("boy,by->o", p.dy[:, :, :, 132].double(), v)
    assert float(delta.abs().max()) > 0
    _flagged(O.check(p.old.double() + p.dw + delta, *bound), "stale dy in pixels [npx, roundup16(npx))", case)


def test_wrong_fused_apply_uses_s2_for_s1():
    p = SC.fused_problem("6x300", 32, 1)
    red = SC.fused_red(p, 4)
    f = SC.fused_ref(p, red)
    tgt, b = O.fused_dw_bound(f, p.P, p.n, p.old_dw)
    assert O.check(fused_dw32(p, fused_dz32(p, red)), tgt, b)[1] == 0
    _flagged(O.check(fused_dw32(p, fused_dz32(p, red, swap=True)), tgt, b), "S2 where S1 belongs", "6x300 c32 s1 slots 4")
