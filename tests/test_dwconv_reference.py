"""oracle/dwconv.py, the fp64 reference of the depthwise convolution and its derived per-element bounds (no GPU), at every
case of the matrix tests/test_gpu_dwconv_elements.py runs on the GPU (tests/dwconv_cases.py):
  * the reference is torch.nn.functional.conv2d(groups=C) and its autograd in float64, to 1e-12 relative;
  * a correct fp32 implementation (torch fp32 conv2d + autograd, rounded to the storage type) stays inside every bound;
  * the bounds are not vacuous: each of seven plausible kernel mistakes is flagged at every case where it applies;
  * every weight-gradient case has n^2 u <= 1/4, so that the bound stays below a quarter of a mean product."""
import functools

import pytest
import torch
import torch.nn.functional as F

from dwconv_cases import ACTS, BY_ID, CASES, CONST_SHAPE, act_fn, const_problem, dead_tail, dtypes_of, matrix, out_hw, pre_inputs, problem
from oracle import dwconv as O

ALL = sorted({(c.id, dt) for c in CASES for op in c.ops for dt in dtypes_of(c, op)})
SENTINEL = 1984.0


def _oihw(w, k):
    return w.t().reshape(w.shape[1], 1, k, k).contiguous()


@functools.lru_cache(maxsize=None)
def emulation(case_id, dt):
    """torch fp32 conv2d + autograd: (y32, dx32, dw32 tap-major) -- the unrounded fp32 results of a correct implementation"""
    p = problem(case_id, dt)
    c = p.case
    x = p.x.clone().requires_grad_(True)
    w = _oihw(p.w, c.k).requires_grad_(True)
    y = F.conv2d(x, w, stride=c.s, padding=c.pad, groups=c.C)
    y.backward(p.dy)
    return y.detach(), x.grad, w.grad.reshape(c.C, c.k * c.k).t().contiguous()


@pytest.mark.parametrize("case_id", [c.id for c in CASES])
def test_reference_is_conv2d_in_float64(case_id):
    p = problem(case_id, "f32")
    c, r = p.case, p.ref
    x = p.x.double().requires_grad_(True)
    w = _oihw(p.w.double(), c.k).requires_grad_(True)
    y = F.conv2d(x, w, stride=c.s, padding=c.pad, groups=c.C)
    y.backward(p.dy.double())
    for name, got, ref in (("y", r.y, y.detach()), ("dx", r.dx, x.grad), ("dw", r.dw, w.grad.reshape(c.C, -1).t())):
        assert got.shape == ref.shape, name
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), name
    assert torch.allclose(r.S1, y.detach().sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r.S2, (y.detach() ** 2).sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    # the absolute-value companions: the same sums over |x|, |w|, |dy|
    ya = F.conv2d(p.x.double().abs(), _oihw(p.w.double().abs(), c.k), stride=c.s, padding=c.pad, groups=c.C)
    assert torch.allclose(r.A_y, ya, rtol=1e-12, atol=1e-12)
    assert bool((r.A_dw >= r.dw.abs() * (1 - 1e-12)).all()) and bool((r.A_dx >= r.dx.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("case_id,dt", ALL)
def test_fp32_emulation_stays_inside_every_bound(case_id, dt):
    p = problem(case_id, dt)
    c, r, T = p.case, p.ref, p.case.k ** 2
    y32, dx32, dw32 = emulation(case_id, dt)
    ratios = {}
    tgt, b = O.out_bound(r.y, r.A_y, T, p.dtype)
    ratios["y"], bad = O.check(O.store(y32, p.dtype), tgt, b)
    assert bad == 0
    b1, b2 = O.stats_bound(r)
    ratios["s1"], bad1 = O.check(y32.sum((0, 2, 3)), r.S1, b1)
    ratios["s2"], bad2 = O.check((y32 * y32).sum((0, 2, 3)), r.S2, b2)
    assert bad1 == 0 and bad2 == 0
    tgt, b = O.out_bound(r.dx, r.A_dx, T, p.dtype)
    ratios["dx"], bad = O.check(O.store(dx32, p.dtype), tgt, b)
    assert bad == 0
    tgt, b = O.out_bound(r.dx, r.A_dx, T, p.dtype, old=p.old)
    ratios["dx+"], bad = O.check(O.store(p.old + dx32, p.dtype), tgt, b)
    assert bad == 0
    ratios["dw"], bad = O.check(dw32, r.dw, O.dw_bound(r))
    assert bad == 0
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("case_id", [c.id for c in CASES if "w" in c.ops])
def test_weight_gradient_cases_keep_a_single_pixel_visible(case_id):
    """n^2 u <= 1/4: the bound (n + 1) u A_dw ~ n^2 u mean|dy x| stays below a quarter of a mean product"""
    r = problem(case_id, "f32").ref
    assert r.n <= 2048 and r.n * r.n * O.U <= 0.25


# ------------------------------------------------------------------ mutants: what a subtly wrong kernel would store
def _truncate(t32, dtype):
    """round towards zero onto the storage grid"""
    v = t32.double()
    u = O.ulp(v, dtype)
    return torch.sign(v) * torch.floor(v.abs() / u) * u


@pytest.mark.parametrize("case_id,dt", [(i, d) for i, d in ALL if d != "f32"])
def test_mutant_truncating_store(case_id, dt):
    p = problem(case_id, dt)
    r, T = p.ref, p.case.k ** 2
    y32, dx32, _ = emulation(case_id, dt)
    tgt, b = O.out_bound(r.y, r.A_y, T, p.dtype)
    assert O.check(_truncate(y32, p.dtype), tgt, b)[1] > 0
    tgt, b = O.out_bound(r.dx, r.A_dx, T, p.dtype)
    assert O.check(_truncate(dx32, p.dtype), tgt, b)[1] > 0


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2)])
def test_mutant_statistics_from_stored_values(k, stride):
    p = const_problem(k, stride)
    r = p.ref
    y32 = F.conv2d(p.x, _oihw(p.w, k), stride=stride, padding=k // 2, groups=CONST_SHAPE[1])
    b1, b2 = O.stats_bound(r)
    assert O.check(y32.sum((0, 2, 3)), r.S1, b1)[1] == 0 and O.check((y32 * y32).sum((0, 2, 3)), r.S2, b2)[1] == 0
    st = y32.bfloat16().double()
    r1, bad1 = O.check(st.sum((0, 2, 3)), r.S1, b1)
    r2, bad2 = O.check((st * st).sum((0, 2, 3)), r.S2, b2)
    assert bad1 == CONST_SHAPE[1] and bad2 == CONST_SHAPE[1] and r1 > 10 and r2 > 20, (r1, r2)


@pytest.mark.parametrize("case_id,dt", ALL)
def test_mutant_dropped_tap_at_one_column(case_id, dt):
    """the centre tap (always inside the image here: pad <= (k - 1) / 2 or the column is interior) left out at output column Wo / 2"""
    p = problem(case_id, dt)
    c, r, T = p.case, p.ref, p.case.k ** 2
    y32 = emulation(case_id, dt)[0].clone()
    Ho, Wo = out_hw(c)
    kh = kw = c.k // 2
    xo = Wo // 2
    xp = F.pad(p.x, (c.pad,) * 4)
    contrib = xp[:, :, kh:kh + (Ho - 1) * c.s + 1:c.s, xo * c.s + kw] * p.w[kh * c.k + kw].view(1, -1, 1)
    assert float(contrib.abs().max()) > 0
    y32[:, :, :, xo] -= contrib
    tgt, b = O.out_bound(r.y, r.A_y, T, p.dtype)
    assert O.check(O.store(y32, p.dtype), tgt, b)[1] > 0


@pytest.mark.parametrize("case_id,dt", [(i, d) for i, d in ALL if BY_ID[i].k > 1 and BY_ID[i].H * BY_ID[i].W > 1])
def test_mutant_taps_not_flipped_in_the_data_gradient(case_id, dt):
    """the forward correlation applied to dy instead of the flipped one (weights are random, hence asymmetric)"""
    p = problem(case_id, dt)
    c, r, T = p.case, p.ref, p.case.k ** 2
    wrong = torch.nn.grad.conv2d_input(p.x.shape, _oihw(p.w.flip(0), c.k), p.dy, stride=c.s, padding=c.pad, groups=c.C)
    tgt, b = O.out_bound(r.dx, r.A_dx, T, p.dtype)
    assert O.check(O.store(wrong, p.dtype), tgt, b)[1] > 0


DEAD = [c for c in CASES if "d" in c.ops and max(dead_tail(c)) > 0]


def test_matrix_has_rows_and_columns_without_gradient():
    """stride 2 at k 3 and k 5 (dwconv_s2_dgrad_kernel), and stride 3 (generic kernel)"""
    assert {(c.k, c.s) for c in DEAD if dead_tail(c)[0]} >= {(3, 2), (5, 2), (3, 3)}
    assert {(c.k, c.s) for c in DEAD if dead_tail(c)[1]} >= {(3, 2), (5, 2)}
    for c in CASES:
        if "d" in c.ops:
            A = problem(c.id, "f32").ref.A_dx
            rows, cols = dead_tail(c)
            assert int((A == 0).sum()) == c.B * c.C * (c.H * c.W - (c.H - rows) * (c.W - cols)), c.id


@pytest.mark.parametrize("case_id,dt", [(c.id, d) for c in DEAD for d in dtypes_of(c, "d")])
def test_mutant_rows_without_gradient_left_unwritten(case_id, dt):
    p = problem(case_id, dt)
    r, T = p.ref, p.case.k ** 2
    dead = (r.A_dx == 0)
    assert bool(dead.any())
    dx = O.store(emulation(case_id, dt)[1], p.dtype).double()
    tgt, b = O.out_bound(r.dx, r.A_dx, T, p.dtype)
    assert O.check(dx, tgt, b)[1] == 0 and bool((dx[dead] == 0).all())
    dx[dead] = SENTINEL
    assert O.check(dx, tgt, b)[1] == int(dead.sum())


@pytest.mark.parametrize("case_id,dt", [(i, d) for i, d in matrix("w")])
def test_mutant_row_or_pixel_left_out_of_the_weight_gradient(case_id, dt):
    p = problem(case_id, dt)
    c, r = p.case, p.ref
    dw32 = emulation(case_id, dt)[2]
    Ho, Wo = out_hw(c)
    xp = F.pad(p.x, (c.pad,) * 4)
    b, yo, xo = c.B - 1, Ho // 2, Wo // 2
    row = torch.zeros_like(dw32)
    pix = torch.zeros_like(dw32)
    for kh in range(c.k):
        for kw in range(c.k):
            t = kh * c.k + kw
            row[t] = (p.dy[b, :, yo, :] * xp[b, :, yo * c.s + kh, kw:kw + (Wo - 1) * c.s + 1:c.s]).sum(1)
            pix[t] = p.dy[b, :, yo, xo] * xp[b, :, yo * c.s + kh, xo * c.s + kw]
    bound = O.dw_bound(r)
    assert O.check(dw32 - row, r.dw, bound)[1] > 0
    assert O.check(dw32 - pix, r.dw, bound)[1] > 0


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("k", [3, 5])
def test_mutant_pre_padding_with_act_of_shift(act, k):
    """normalise-on-load must pad the NORMALISED tensor with 0, not normalise the zero padding of the raw one"""
    B, C, H, W = 2, 72, 11, 19
    pad = k // 2
    u, scale, shift = pre_inputs(C, B, H, W, 7)
    g = torch.Generator().manual_seed(8)
    w = torch.randn(k * k, C, generator=g) / k
    fn = act_fn(act)
    z = fn(u * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).bfloat16().float()
    r = O.reference(z, w, None, k, 1, pad)
    tgt, b = O.out_bound(r.y, r.A_y, k * k, torch.bfloat16)
    good = F.conv2d(z, _oihw(w, k), padding=pad, groups=C)
    assert O.check(O.store(good, torch.bfloat16), tgt, b)[1] == 0
    zp = fn(shift).bfloat16().float().view(1, -1, 1, 1).expand(B, C, H + 2 * pad, W + 2 * pad).clone()
    zp[:, :, pad:pad + H, pad:pad + W] = z
    wrong = F.conv2d(zp, _oihw(w, k), groups=C)
    ratio, bad = O.check(O.store(wrong, torch.bfloat16), tgt, b)
    border = 2 * (H + W) - 4
    assert bad >= B * C * border // 2 and ratio > 50, (ratio, bad)
