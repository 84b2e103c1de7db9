"""oracle/elementwise.py, the fp64 reference of the kernels of csrc/elementwise.hip and its derived per-element bounds (no GPU), at the
cases tests/test_gpu_elementwise_elements.py runs on the GPU (tests/elementwise_cases.py):
  * the oracle's max-pool rule (first maximum, last NaN, window start when everything is -inf) is torch's CPU
    max_pool2d(..., return_indices=True) on the whole pool matrix, special values included, in fp32, bf16 and fp64;
  * fp32 emulations of the kernels' arithmetic written in torch stay inside every bound: the separable row-then-column forward of the
    tile kernels (which yields exactly the oracle's values and codes), their two-stage backward, the k * k gather of the generic kernels,
    and the per-thread chains of dot, se_pool, dot16 / the SE matrix-vector launches and the head bias gradient under the restated
    launch geometry -- each prints `EWEMU <what> <largest error / bound> <case>`;
  * the bounds are not vacuous: each of a list of wrong kernels is flagged by a named case;
  * the path assertions of the cases file hold for every case."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_cases as EC
from oracle import elementwise as O

F32 = torch.float32
NAN = float("nan")


def _report(what, ratio, bad, case):
    print("EWEMU %s %.5f %s" % (what, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s: %d elements outside their bound, largest error / bound %.3f" % (what, case, bad, ratio)


def _flagged(bad, what, case):
    assert bad > 0, "%s is NOT flagged by case %s" % (what, case)


def _pool_cases():
    """(B, C, H, W, k, stride) of every pool launch of the GPU file"""
    out = [(B, C, H, W, k, 1) for (H, W, k) in EC.tile_matrix() for (dt, C, B, lay) in EC.tile_variants(H, W, k)]
    out += [(1, C, 33, 32, k, 1) for k in EC.GENERIC_KS for C in (8, 4, 24)]
    out += [(2, C, H, W, k, s) for (k, s) in EC.STRIDED for (H, W) in EC.STRIDED_MAPS for C in (8, 4, 16)]
    return sorted(set(out))


# ---------------------------------------------------------------------------------------------------- the pool rule is torch's
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64], ids=["f32", "bf16", "f64"])
def test_pool_rule_is_torch_max_pool2d(dtype):
    refused = 0
    for (B, C, H, W, k, s) in _pool_cases() + [(1, 8) + EC.BIG_POOL + (3, 1)]:
        if dtype != torch.float32 and H * W > 4096:
            continue
        x = EC.pool_input(B, C, H, W)
        pad = (k - 1) // 2
        if 0 in EC.pool_shape(H, W, k, s):
            with pytest.raises(RuntimeError):
                F.max_pool2d(x, k, s, pad)
            refused += 1
            continue
        v, c = EC.pool_ref(B, C, H, W, k, s)
        tv, ti = F.max_pool2d(x.to(dtype), k, s, pad, return_indices=True)
        assert v.shape == tv.shape and int(c.max()) <= 224
        assert O.same_bits(tv, v.to(dtype)) == 0, (B, C, H, W, k, s)
        assert torch.equal(ti, O.code_index(c, k, s, H, W)), (B, C, H, W, k, s)
    assert refused > 0                                 # (an even window on the one-pixel map)


def test_the_package_sizes_pool_outputs_as_the_oracle_and_refuses_empty_maps():
    """dyk.ops.maxpool_out_size, where dyk.functional.maxpool and the plan compiler size a pool's output: the oracle's extent, and a
    ValueError where torch raises -- the kernels' own truncating division would make (k 2, stride 2) on one pixel ONE output"""
    from dyk import ops
    refused = set()
    for (B, C, H, W, k, s) in _pool_cases():
        for n in (H, W):
            want = O.pool_out(n, k, s)
            if want == 0:
                with pytest.raises(ValueError):
                    ops.maxpool_out_size(n, k, s)
                refused.add((n, k, s))
            else:
                assert ops.maxpool_out_size(n, k, s) == want
    assert refused == {(1, 2, 2), (1, 4, 1), (1, 2, 1)}
    assert int((1 + 0 - 2) / 2) + 1 == 1               # what C's division gives for (1, 2, 2)


def test_pool_input_holds_every_special_value():
    x = EC.pool_input(3, 8, 7, 9)
    assert int(torch.isnan(x[0, 0]).sum()) == 1 and int(torch.isnan(x[0, 1]).sum()) == 4 and bool(torch.isinf(x[0, 2]).any())
    assert bool((x[0, 3] == float("-inf")).all())
    z = x[2, 2][x[2, 2] == 0]
    assert bool(torch.signbit(z).any()) and bool((~torch.signbit(z)).any())
    v, c = EC.pool_ref(3, 8, 7, 9, 3, 1)
    assert bool(torch.isnan(v[0, 1, 0, 0])) and int(c[0, 1, 0, 0]) == 2 * 3 + 1              # the LAST NaN of the window: pixel (1, 0) -> dy 2, dx 1
    assert bool((c[0, 3, 1:-1, 1:-1] == 0).all()) and int(c[0, 3, 0, 0]) == 4                # all -inf: the window's first tap


# ---------------------------------------------------------------------------------------------------- pool emulations
RULES = {
    "right": lambda t, m: (t > m) | torch.isnan(t),
    ">= instead of > (last tie)": lambda t, m: (t >= m) | torch.isnan(t),
    "the first NaN kept": lambda t, m: (t > m) | (torch.isnan(t) & ~torch.isnan(m)),
    "NaN ignored": lambda t, m: t > m,
}


def _scan1d(v, k, dim, rule, aux=None, own_aux=False, clamp_counts=False):
    """one pass of the separable forward along `dim`: (maximum, index of the selected tap, aux of the selected tap).  Loads are clamped
    to the map as the kernel's are; a validity bit decides whether a tap counts"""
    n, pad = v.shape[dim], (k - 1) // 2
    shape = [1, 1, 1, 1]
    shape[dim] = n
    m = torch.full_like(v, float("-inf"))
    pos = torch.zeros(v.shape, dtype=torch.long)
    sel_aux = torch.zeros(v.shape, dtype=torch.long)
    seen = torch.zeros(shape, dtype=torch.bool)
    for d in range(k):
        idx = torch.arange(n) + d - pad
        ok = ((idx >= 0) & (idx < n)).view(shape)
        if clamp_counts:
            ok = torch.ones_like(ok)
        idx = idx.clamp(0, n - 1)
        tap = v.index_select(dim, idx)
        take = ok & (~seen | rule(tap, m))
        m = torch.where(take, tap, m)
        pos = torch.where(take, torch.full_like(pos, d), pos)
        if aux is not None:
            sel_aux = torch.where(take, aux if own_aux else aux.index_select(dim, idx), sel_aux)
        seen = seen | ok
    return m, pos, sel_aux


def tile_forward(x, k, rule="right", code_width=None, own_row_dx=False, clamp_counts=False):
    """maxpool_tile_fwd_kernel: the row pass (maximum of each window row and its dx), then the column pass over the row results"""
    rmax, radx, _ = _scan1d(x.float(), k, 3, RULES[rule], clamp_counts=clamp_counts)
    m, dy, dx = _scan1d(rmax, k, 2, RULES[rule], aux=radx, own_aux=own_row_dx, clamp_counts=clamp_counts)
    return m, (dy * (code_width or k) + dx).to(torch.uint8)


def generic_backward(g, code, k, stride, H, W, old=None, rows=None):
    """maxpool_bwd_kernel: every input gathers over the window positions in (dy, dx) order, fp32"""
    B, C, Ho, Wo = g.shape
    pad = (k - 1) // 2
    ye, xe = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1
    s = torch.zeros(B, C, max(H + pad, ye + k - 1), max(W + pad, xe + k - 1), dtype=F32)
    zero = torch.zeros((), dtype=F32)
    for dy in range(k if rows is None else rows):
        for dx in range(k):
            s[:, :, dy:dy + ye:stride, dx:dx + xe:stride] += torch.where(code == dy * k + dx, g, zero)
    s = s[:, :, pad:pad + H, pad:pad + W]
    return s if old is None else s + old


def tile_backward(g, code, k, old=None, rows=None):
    """maxpool_tile_bwd_kernel: stage 1 sums, per (row, column) of the row-window results, the outputs above / below whose code selects
    that row, keeping their dx; stage 2 sums the row-window results left / right whose dx points at the input.  fp32"""
    B, C, H, W = g.shape
    pad = (k - 1) // 2
    code = code.long()
    zero = torch.zeros((), dtype=F32)
    r = torch.zeros(B, C, H + 2 * pad, W, dtype=F32)
    rd = torch.full((B, C, H + 2 * pad, W), 255, dtype=torch.long)
    for dy in range(k if rows is None else rows):
        sel = (code >= dy * k) & (code < dy * k + k)
        r[:, :, dy:dy + H] += torch.where(sel, g, zero)
        rd[:, :, dy:dy + H] = torch.where(sel, code - dy * k, rd[:, :, dy:dy + H])
    r, rd = r[:, :, pad:pad + H], rd[:, :, pad:pad + H]
    s = torch.zeros(B, C, H, W + 2 * pad, dtype=F32)
    for dx in range(k):
        s[..., dx:dx + W] += torch.where(rd == dx, r, zero)
    s = s[..., pad:pad + W]
    return s if old is None else s + old


def _check_backward(B, C, H, W, k, s, dt, emu, what, case):
    for nan, acc in ((False, False), (False, True), (True, False)):
        dy, old, tgt, bound = EC.pool_bwd_ref(B, C, H, W, k, s, dt, nan, acc)
        got = O.store(emu(dy, old), EC.DTYPES[dt])
        _report("%s%s%s-%s" % (what, "-accum" if acc else "", "-nan" if nan else "", dt), *O.check_nan(got, tgt, bound), case)


@pytest.mark.parametrize("H,W,k", EC.tile_matrix())
def test_separable_emulations_give_the_oracle(H, W, k):
    """forward: exactly the oracle's values and codes, NaN and tie cases included; backward: inside the bound, NaN gradients at exactly
    the selected inputs"""
    for dt, C, B, lay in EC.tile_variants(H, W, k):
        case = "tile %dx%d k%d c%d b%d" % (H, W, k, C, B)
        v, c = EC.pool_ref(B, C, H, W, k, 1)
        ev, ec = tile_forward(EC.pool_input(B, C, H, W), k)
        assert O.same_bits(ev, v) == 0 and torch.equal(ec, c), case
        if dt != "f16":
            _check_backward(B, C, H, W, k, 1, dt, lambda g, old: tile_backward(g, c, k, old), "tile-bwd", case)
            _check_backward(B, C, H, W, k, 1, dt, lambda g, old: generic_backward(g, c, k, 1, H, W, old), "gather-bwd", case)


@pytest.mark.parametrize("k,s", [(kk, 1) for kk in EC.GENERIC_KS] + EC.STRIDED)
def test_gather_emulation_on_the_generic_and_strided_cases(k, s):
    maps = [EC.GENERIC_MAP] if (k, s) in [(kk, 1) for kk in EC.GENERIC_KS] else EC.STRIDED_MAPS
    for (H, W) in maps:
        if 0 in EC.pool_shape(H, W, k, s):
            continue
        for dt, C in (("bf16", 8), ("f32", 4)):
            B = 1 if H * W > 1024 else 2
            c = EC.pool_ref(B, C, H, W, k, s)[1]
            _check_backward(B, C, H, W, k, s, dt, lambda g, old: generic_backward(g, c, k, s, H, W, old), "gather-bwd",
                            "%dx%d k%d s%d c%d" % (H, W, k, s, C))


# each wrong pool kernel and the case that must flag it: (what, (B, C, H, W, k), keyword arguments of tile_forward)
POOL_MUTANTS = [
    (">= instead of > (last tie)", (3, 8, 7, 9, 3), dict(rule=">= instead of > (last tie)")),
    ("the first NaN kept", (3, 8, 7, 9, 3), dict(rule="the first NaN kept")),
    ("NaN ignored", (3, 8, 7, 9, 5), dict(rule="NaN ignored")),
    ("a code with W instead of k", (3, 24, 16, 20, 5), dict(code_width=20)),
    ("the column pass taking dx from the output's own row", (3, 8, 7, 9, 5), dict(own_row_dx=True)),
    ("a clamped tap counted", (3, 8, 2, 3, 13), dict(clamp_counts=True)),
]


@pytest.mark.parametrize("what,shape,kw", POOL_MUTANTS, ids=[m[0] for m in POOL_MUTANTS])
def test_wrong_pool_forward_is_flagged(what, shape, kw):
    B, C, H, W, k = shape
    assert (H, W, k) in EC.tile_matrix()
    v, c = EC.pool_ref(B, C, H, W, k, 1)
    ev, ec = tile_forward(EC.pool_input(B, C, H, W), k, **kw)
    _flagged(O.same_bits(ev, v) + int((ec != c).sum()), what, "tile %dx%d k%d" % (H, W, k))


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_wrong_pool_backward_is_flagged(dt):
    B, C, H, W, k = 3, {"bf16": 8, "f32": 4}[dt], 7, 9, 5
    c = EC.pool_ref(B, C, H, W, k, 1)[1]
    case = "tile 7x9 k5 %s" % dt
    dy, old, tgt, bound = EC.pool_bwd_ref(B, C, H, W, k, 1, dt, False, False)
    for emu in (tile_backward, lambda g, cc, kk, rows: generic_backward(g, cc, kk, 1, H, W, rows=rows)):
        got = O.store(emu(dy, c, k, rows=k - 1), EC.DTYPES[dt])
        _flagged(O.check_nan(got, tgt, bound)[1], "the backward dropping the last window row", case)
    dy, old, tgt, bound = EC.pool_bwd_ref(B, C, H, W, k, 1, dt, False, True)
    _flagged(O.check_nan(O.store(tile_backward(dy, c, k), EC.DTYPES[dt]), tgt, bound)[1], "accumulate ignored", case)
    # a NaN gradient must reach exactly the selected input: a kernel that multiplies by a 0 / 1 mask instead of selecting spreads it
    dy, old, tgt, bound = EC.pool_bwd_ref(B, C, H, W, k, 1, dt, True, False)
    spread = generic_backward(dy, c, k, 1, H, W) + 0.0 * F.max_pool2d(dy, k, 1, (k - 1) // 2)
    _flagged(O.check_nan(O.store(spread, EC.DTYPES[dt]), tgt, bound)[1], "a NaN gradient spread over the window", case)


# ---------------------------------------------------------------------------------------------------- upsample, axpby, dot
def up_backward(g, old=None, taps=4):
    t = [g[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)][:taps]
    s = t[0]
    for v in t[1:]:
        s = s + v
    return s if old is None else s + old


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_upsample_emulation_and_mutants(dt):
    B, C, H, W = 2, 8, 7, 9
    x = EC.rand_tensor(B, C, H, W, dt, 1)
    up = O.up_fwd(x)
    assert up.shape == (B, C, 2 * H, 2 * W) and torch.equal(up, F.interpolate(x, scale_factor=2, mode="nearest"))
    g, old = EC.rand_tensor(B, C, 2 * H, 2 * W, dt, 2), EC.rand_tensor(B, C, H, W, dt, 3)
    for o in (None, old):
        tgt, bound = O.up_bwd(g, EC.DTYPES[dt], o)
        _report("up-bwd-" + dt, *O.check(O.store(up_backward(g, o), EC.DTYPES[dt]), tgt, bound), "7x9 c8 acc=%d" % (o is not None))
        _flagged(O.check(O.store(up_backward(g, o, taps=3), EC.DTYPES[dt]), tgt, bound)[1], "upsample backward missing the (1,1) tap", "7x9 c8 " + dt)
    tgt, bound = O.up_bwd(g, EC.DTYPES[dt], old)
    _flagged(O.check(O.store(up_backward(g), EC.DTYPES[dt]), tgt, bound)[1], "accumulate ignored", "7x9 c8 " + dt)
    xr = x.double().requires_grad_(True)
    F.interpolate(xr, scale_factor=2, mode="nearest").backward(g.double())
    assert torch.allclose(O.up_bwd(g, torch.float32)[0], xr.grad, rtol=1e-13, atol=0)


def _fma(a, b, c):
    """a * b + c with one rounding (float32 operands: the product is exact in float64)"""
    return (a.double() * b.double() + c.double()).float()


def axpby32(a, alpha, beta, b, p0, p1, old, fused):
    one = torch.tensor(1.0)
    sa = torch.tensor(alpha, dtype=F32) * (one if p0 is None else torch.tensor(p0, dtype=F32))
    sb = torch.tensor(beta, dtype=F32) * (one if p1 is None else torch.tensor(p1, dtype=F32))
    x = a * sa if alpha != 0 else torch.zeros_like(a)
    if b is not None:
        x = _fma(sb, b, x) if fused else x + sb * b
    return x if old is None else x + old


@pytest.mark.parametrize("dt", ["bf16", "f32", "f16"])
def test_axpby_emulations_and_mutants(dt):
    B, C, H, W = 2, 24, 3, 5
    a, b, old = (EC.rand_tensor(B, C, H, W, dt, s) for s in (11, 12, 13))
    dtype = EC.DTYPES[dt]
    for form in EC.AXPBY_FORMS:
        has_b, has_p0, has_p1, acc, in_place = form
        o = (a if in_place else old) if acc else None
        args = (0.75, -1.25, b if has_b else None, 1.5 if has_p0 else None, 0.3 if has_p1 else None, o)
        tgt, bound = O.axpby(a, dtype, *args)
        for fused in (False, True):
            _report("axpby-%s-%s" % ("fused" if fused else "unfused", dt), *O.check(O.store(axpby32(a, *args, fused), dtype), tgt, bound), str(form))
        if acc:
            wrong = axpby32(a, *args[:5], None, True)
            _flagged(O.check(O.store(wrong, dtype), tgt, bound)[1], "accumulate ignored", "axpby %s %s" % (dt, form))
    # alpha = 0: an exact zero whatever `a` holds; a kernel that multiplies is flagged
    nanbuf = torch.full_like(a, NAN)
    tgt, bound = O.axpby(nanbuf, dtype, 0.0, -1.25, b)
    _report("axpby-alpha0-" + dt, *O.check(O.store(axpby32(nanbuf, 0.0, -1.25, b, None, None, None, True), dtype), tgt, bound), "NaN buffer")
    _flagged(O.check(O.store(nanbuf * 0.0 + b * -1.25, dtype), tgt, bound)[1], "alpha = 0 multiplied into `a`", "axpby " + dt)
    if dt == "f32":          # a plain copy is exact
        tgt, bound = O.axpby(a, dtype)
        assert float(bound.max()) == 0.0 and torch.equal(tgt.float(), a)


def dot32(a, b, dt, fused):
    """dot_kernel: vector v goes to thread v % (G * 256); per thread a chain over its trips and the EPV elements; wave fold, 4-wave fold;
    the workgroup sums added in fp64"""
    epv = EC.epv(dt)
    av, bv = (t.permute(0, 2, 3, 1).reshape(-1, epv) for t in (a, b))
    vecs = av.shape[0]
    G, trips = EC.dot_grid(vecs), EC.dot_trips(vecs)
    T = G * 256
    padn = trips * T - vecs
    av, bv = (torch.cat([t, torch.zeros(padn, epv)]).view(trips, T, epv) for t in (av, bv))
    s = torch.zeros(T)
    for t in range(trips):
        for j in range(epv):
            s = _fma(av[t, :, j], bv[t, :, j], s) if fused else s + av[t, :, j] * bv[t, :, j]
    s = s.view(G, 4, 64)
    o = 32
    while o:
        s = s[..., :o] + s[..., o:]
        o //= 2
    s = s[..., 0]
    wg = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    return wg.double().sum()


@pytest.mark.parametrize("dt,shape", [("bf16", (2, 24, 3, 5)), ("f32", (2, 12, 3, 5)), ("bf16", (1, 8, 257, 2048))])
def test_dot_emulation(dt, shape):
    """the small cases and one past the 1024-workgroup cap (two to three trips per thread)"""
    a, b = EC.rand_tensor(*shape, dt, 31), EC.rand_tensor(*shape, dt, 32)
    vecs = a.numel() // EC.epv(dt)
    tgt, bound = O.dot(a, b, EC.epv(dt), EC.dot_trips(vecs), EC.dot_grid(vecs))
    for fused in (False, True):
        got = dot32(a, b, dt, fused)
        _report("dot-%s-%s" % ("fused" if fused else "unfused", dt), *O.check(got.view(1), tgt.view(1), torch.tensor([bound])), str(shape))
    half = dot32(a[:, :, :, :shape[3] // 2], b[:, :, :, :shape[3] // 2], dt, True)
    _flagged(O.check(half.view(1), tgt.view(1), torch.tensor([bound]))[1], "dot over half the columns", str(shape))


@pytest.mark.parametrize("n", EC.WFUSE_N)
def test_weighted_fusion_bounds(n):
    """the bound is four times the measured figure rounded up to a power of two; torch's fp32 sigmoid (correct to an ulp or two) is well
    inside it; sigmoid(w) / n for 2 / n, and the derivative without its (1 - s), are flagged"""
    assert O.EXPF_ULPS == 2.0 ** math.ceil(math.log2(4 * O.EXPF_MEASURED))
    w, red, old = EC.wfuse_problem(n)
    s = torch.sigmoid(w)
    two_n = torch.tensor(2.0) / n
    tgt, bound = O.wfuse_weights(w)
    _report("wfuse-weights", *O.check(s * two_n, tgt, bound), "n=%d" % n)
    assert torch.allclose(tgt, torch.sigmoid(w.double()) * 2 / n, rtol=1e-15)
    _flagged(O.check(s / n, tgt, bound)[1], "1 / n for 2 / n", "n=%d" % n)
    tgt, bound = O.wfuse_bwd(w, red, old)
    _report("wfuse-bwd", *O.check(old + red.float() * two_n * s * (1 - s), tgt, bound), "n=%d" % n)
    wr = w.double().requires_grad_(True)
    (torch.sigmoid(wr) * (2.0 / n) * red).sum().backward()
    assert torch.allclose(tgt, old.double() + wr.grad, rtol=1e-12, atol=1e-15)
    if n > 2:                                          # (w = 0 is among the points: s (1 - s) = 1/4 against s = 1/2)
        _flagged(O.check(old + red.float() * two_n * s, tgt, bound)[1], "the derivative without (1 - s)", "n=%d" % n)


# ---------------------------------------------------------------------------------------------------- se_pool
def se_pool32(x, y, alpha, geo, drop_tail=False, fold_from=0):
    """se_pool_kernel + se_pool_fold_kernel: part z takes pixels [z * chunk, min(HW, (z + 1) * chunk)), lane ty those at ty + j * PY in
    turn; lane sums folded in lane order, planes in z order, then alpha.  One channel per column, every channel alike"""
    CVB, PY, gx, HS, chunk = geo
    B, C, H, W = x.shape
    v = (x if y is None else x * y).reshape(B, C, H * W)
    HW = H * W
    planes = []
    for z in range(HS):
        pbeg, pend = z * chunk, min(HW, (z + 1) * chunk)
        if drop_tail:
            pend = pbeg + (pend - pbeg) // PY * PY
        lanes = []
        for ty in range(PY):
            s = torch.zeros(B, C)
            for p in range(pbeg + ty, pend, PY):
                s = s + v[:, :, p]
            lanes.append(s)
        s = lanes[0]
        for q in range(1, PY):
            s = s + lanes[q]
        planes.append(s)
    planes.append(torch.full((B, C), NAN))             # what the scratch holds behind the last plane
    if HS == 1:
        return planes[0] * alpha
    t = torch.zeros(B, C)
    for z in range(fold_from, fold_from + HS):
        t = t + planes[z]
    return t * alpha


@pytest.mark.parametrize("H,W", EC.SE_POOL_MAPS[:4])
@pytest.mark.parametrize("dt,C", EC.SE_POOL_C)
def test_se_pool_emulation_and_mutants(dt, C, H, W):
    B, HW = 2, H * W
    x, y = EC.rand_tensor(B, C, H, W, dt, 41)[:, :8], EC.rand_tensor(B, C, H, W, dt, 42)[:, :8]      # (every channel alike: 8 suffice)
    for second, scratch in ((False, False), (False, True), (True, True)):
        geo = EC.se_pool_geo(C, dt, B, HW, scratch)
        alpha = 0.5 if second else 1.0 / HW
        tgt, bound = O.se_pool(x, alpha, EC.se_pool_m(C, dt, B, HW, scratch), y if second else None)
        case = "%dx%d c%d b=%d CVB%d HS%d" % (H, W, C, second, geo[0], geo[3])
        _report("se_pool-" + dt, *O.check(se_pool32(x, y if second else None, torch.tensor(alpha, dtype=F32), geo), tgt, bound), case)
    if (dt, C, (H, W)) == ("bf16", 136, (43, 49)):
        geo = EC.se_pool_geo(C, dt, B, HW, True)
        assert geo[3] == 16 and geo[4] == 132 and HW - 15 * 132 == 127
        tgt, bound = O.se_pool(x, 1.0 / HW, EC.se_pool_m(C, dt, B, HW, True))
        a = torch.tensor(1.0 / HW, dtype=F32)
        _flagged(O.check(se_pool32(x, None, a, geo, drop_tail=True), tgt, bound)[1], "se_pool dropping a ragged chunk tail", "43x49 c136")
        _flagged(O.check(se_pool32(x, None, a, geo, fold_from=1), tgt, bound)[1], "the fold reading plane HS", "43x49 c136")


def test_se_pool_paths():
    for (dt, C, hw, scratch), (cvb, hs) in EC.SE_POOL_PATHS.items():
        geo = EC.se_pool_geo(C, dt, 2, hw[0] * hw[1], scratch)
        assert (geo[0], geo[3]) == (cvb, hs), (dt, C, hw, scratch, geo)
    assert -(-24 // 8) % 4 != 0 and EC.se_pool_geo(136, "bf16", 2, 272, True)[2] == 2      # CVB 4 with an idle lane; two ragged groups of 16


# ---------------------------------------------------------------------------------------------------- SE FCs
def dot16(Wm, v, mask=True):
    """dot16 for every row of Wm [R, K] and every image of v [B, K] -> [B, R]: lane l takes the float4 at 4 l + 256 t and those 64, 128,
    192 further on (clamped address, zero mask past the end) into four accumulators; (a0 + a1) + (a2 + a3); the 16 lanes as a tree"""
    R, K = Wm.shape
    B = v.shape[0]
    acc = torch.zeros(4, B, R, 16)
    for l in range(16):
        for i in range(l * 4, K, 256):
            for q in range(4):
                iq = i + 64 * q
                live = iq < K
                if not live and mask:
                    continue
                j = iq if live else i
                w, x = Wm[:, j:j + 4], v[:, j:j + 4]
                t = w[None, :, 0] * x[:, None, 0]
                for e in range(1, 4):
                    t = _fma(w[None, :, e], x[:, None, e], t)
                acc[q, :, :, l] = acc[q, :, :, l] + t
    s = (acc[0] + acc[1]) + (acc[2] + acc[3])
    o = 8
    while o:
        s = s[..., :o] + s[..., o:]
        o //= 2
    return s[..., 0]


def rows32(Wm, bias, v, act, slices_wrong=False, R=None):
    """se_rows_kernel under se_rows_grid: every workgroup takes `bper` images; returns (out, pre) with NaN where nothing was written.
    R: the row count of the launch when Wm holds only some of its rows"""
    B = v.shape[0]
    gx, slices, bper = EC.se_rows_grid(R or Wm.shape[0], B)
    t = dot16(Wm, v) + bias
    out = t.clamp(min=0.0) if act == 0 else (t + 3.0).clamp(0.0, 6.0) * torch.tensor(1.0 / 6.0)
    written = torch.zeros(B, dtype=torch.bool)
    for by in range(slices):
        b0 = by * bper
        written[b0:min(B, b0 + bper - (1 if slices_wrong and bper > 1 else 0))] = True
    nan = torch.full_like(out, NAN)
    return torch.where(written[:, None], out, nan), torch.where(written[:, None], t, nan)


def cols32(Wm, v):
    """se_cols_kernel: out[b][k] = sum_r W[r][k] v[b][r]: 16 row groups (r = g, g + 16, ...) each in turn, folded as a tree"""
    R = Wm.shape[0]
    part = []
    for g in range(16):
        acc = torch.zeros(v.shape[0], Wm.shape[1])
        for r in range(g, R, 16):
            acc = _fma(Wm[None, r, :], v[:, r, None], acc)
        part.append(acc)
    w = 8
    while w:
        part = [part[i] + part[i + w] for i in range(w)]
        w //= 2
    return part[0]


def dt2_32(t2, dscale, strict=True):
    live = (t2 > -3.0) & (t2 < 3.0) if strict else (t2 >= -3.0) & (t2 <= 3.0)
    return torch.where(live, dscale * torch.tensor(1.0 / 6.0), torch.zeros_like(t2))


def wgrad32(vb, other, old):
    acc = torch.zeros(vb.shape[1], other.shape[1])
    for b in range(vb.shape[0]):
        acc = _fma(vb[b, :, None], other[b, None, :], acc)
    return old + acc


SE_SMALL = [c for c in EC.SE_FC if c[0] * c[1] * c[2] <= 960 * 240 * 17 and c != (64, 16, 256)]


@pytest.mark.parametrize("C,Cs,B", SE_SMALL)
def test_se_fc_emulations(C, Cs, B):
    p = EC.se_problem(C, Cs, B)
    case = "c%d cs%d b%d" % (C, Cs, B)
    h, _ = rows32(p.w1, p.b1, p.pooled, 0)
    _report("se_fc-h", *O.check(h, *O.se_fc1(p.pooled, p.w1, p.b1)), case)
    scale, t2 = rows32(p.w2, p.b2, h, 1)
    (t_ref, t_b), (s_ref, s_b) = O.se_fc2(h, p.w2, p.b2)
    _report("se_fc-t2", *O.check(t2, t_ref, t_b), case)
    _report("se_fc-scale", *O.check(scale, s_ref, s_b), case)
    s = cols32(p.w2, dt2_32(p.t2, p.dscale))
    dt1 = torch.where(p.h > 0, s, torch.zeros_like(s))
    _report("se_fc-dt1", *O.check(dt1, *O.se_dt1(p.h, p.t2, p.dscale, p.w2)), case)
    _report("se_fc-dpooled", *O.check(cols32(p.w1, dt1), *O.se_dpooled(dt1, p.w1)), case)
    ref = O.se_wgrad(p.pooled, p.h, dt1, p.t2, p.dscale, p.old)
    d2 = dt2_32(p.t2, p.dscale)
    ones = torch.ones(B, 1)
    got = {"dw2": wgrad32(d2, p.h, p.old["dw2"]), "dw1": wgrad32(dt1, p.pooled, p.old["dw1"]),
           "db2": wgrad32(d2, ones, p.old["db2"][:, None])[:, 0], "db1": wgrad32(dt1, ones, p.old["db1"][:, None])[:, 0]}
    for k, v in got.items():
        _report("se_fc-" + k, *O.check(v, *ref[k]), case)


def test_wrong_se_fc_kernels_are_flagged():
    # dot16 without the tail mask: K = 4, the second to fourth loads are all past the end
    p = EC.se_problem(8, 4, 1)
    h = rows32(p.w1, p.b1, p.pooled, 0)[0]
    (t_ref, t_b), _ = O.se_fc2(h, p.w2, p.b2)
    assert float(h.abs().max()) > 0
    _flagged(O.check(dot16(p.w2, h, mask=False) + p.b2, t_ref, t_b)[1], "dot16 without the tail mask", "c8 cs4 b1 (K = 4)")
    p = EC.se_problem(260, 132, 5)
    t_ref, t_b = O.se_fc1(p.pooled, p.w1, p.b1)
    _flagged(O.check((dot16(p.w1, p.pooled, mask=False) + p.b1).clamp(min=0), t_ref, t_b)[1], "dot16 without the tail mask", "c260 cs132 b5 (K = 260)")
    # hard-sigmoid backward with <=: the exact +-3 of the workspace
    _flagged(O.check(torch.where(p.h > 0, cols32(p.w2, dt2_32(p.t2, p.dscale, strict=False)), torch.zeros_like(p.h)),
                     *O.se_dt1(p.h, p.t2, p.dscale, p.w2))[1], "hard-sigmoid backward with <=", "c260 cs132 b5 dt1")
    ref = O.se_wgrad(p.pooled, p.h, p.dt1, p.t2, p.dscale, p.old)
    _flagged(O.check(wgrad32(dt2_32(p.t2, p.dscale, strict=False), p.h, p.old["dw2"]), *ref["dw2"])[1], "hard-sigmoid backward with <=", "c260 cs132 b5 dw2")
    # relu backward with >=: the exact zeros of h
    s = cols32(p.w2, dt2_32(p.t2, p.dscale))
    _flagged(O.check(torch.where(p.h >= 0, s, torch.zeros_like(s)), *O.se_dt1(p.h, p.t2, p.dscale, p.w2))[1], "relu backward with >=", "c260 cs132 b5")
    # the weight gradient overwriting instead of accumulating
    _flagged(O.check(wgrad32(p.dt1, p.pooled, torch.zeros_like(p.old["dw1"])), *ref["dw1"])[1], "weight gradient not accumulated", "c260 cs132 b5")
    # bper slice off by one: the last image of every slice is left unwritten
    for (C, Cs, B) in EC.SE_FC_BPER:
        p = EC.se_problem(C, Cs, B)
        assert EC.se_rows_grid(C, B)[2] == EC.SE_FC_BPER[(C, Cs, B)]
        h = O.se_fc1(p.pooled, p.w1, p.b1)[0].float()
        _, (s_ref, s_b) = O.se_fc2(h, p.w2, p.b2)
        rows = torch.arange(0, C, 30)                                        # (every row alike: the slicing is per image)
        case = "c%d cs%d b%d" % (C, Cs, B)
        _report("se_fc-scale", *O.check(rows32(p.w2[rows], p.b2[rows], h, 1, R=C)[0], s_ref[:, rows], s_b[:, rows]), case)
        _flagged(O.check(rows32(p.w2[rows], p.b2[rows], h, 1, slices_wrong=True, R=C)[0], s_ref[:, rows], s_b[:, rows])[1], "bper slice off by one", case)


def test_se_rows_grid_paths():
    assert EC.se_rows_grid(960, 16) == (60, 8, 2) and EC.se_rows_grid(960, 17) == (60, 6, 3) and 17 - 5 * 3 == 2
    assert EC.se_rows_grid(240, 16)[2] == 1 and EC.se_rows_grid(8192, 1) == (512, 1, 1)
    for (C, Cs, B) in EC.SE_FC:
        for R in (C, Cs):
            gx, slices, bper = EC.se_rows_grid(R, B)
            assert slices * bper >= B > (slices - 1) * bper and (bper > 1) == (gx * B > 512)
    ks = sorted({c[0] for c in EC.SE_FC} | {c[1] for c in EC.SE_FC})
    assert {4, 260, 960} <= set(ks)                    # dot16: one load live; 4 + 1 trips with one live load in the last; 3 + 3 of 4 live


# ---------------------------------------------------------------------------------------------------- se_scale
@pytest.mark.parametrize("dt,C", EC.SE_SCALE_C)
def test_se_scale_emulation_and_paths(dt, C):
    B, H, W = 2, 3, 5
    a, old = EC.rand_tensor(B, C, H, W, dt, 51), EC.rand_tensor(B, C, H, W, dt, 52)
    g = torch.Generator().manual_seed(C + H)
    p0, p1 = torch.rand(B, C, generator=g), torch.randn(B, C, generator=g)
    alpha = torch.tensor(1.0 / (H * W), dtype=F32)
    for has_p1 in (False, True):
        for acc in (False, True):
            tgt, bound = O.se_scale(a, p0, EC.DTYPES[dt], p1 if has_p1 else None, float(alpha), old if acc else None)
            f1 = (p1 * alpha)[:, :, None, None] if has_p1 else torch.zeros(B, C, 1, 1)
            for fused in (False, True):
                x = _fma(a, p0[:, :, None, None], f1) if fused else a * p0[:, :, None, None] + f1
                x = x + old if acc else x
                _report("se_scale-" + dt, *O.check(O.store(x, EC.DTYPES[dt]), tgt, bound), "c%d p1=%d acc=%d fused=%d" % (C, has_p1, acc, fused))
            if acc:
                _flagged(O.check(O.store(a * p0[:, :, None, None] + f1, EC.DTYPES[dt]), tgt, bound)[1], "accumulate ignored", "se_scale c%d" % C)
    Bl, Cl, Hl, Wl = EC.SE_SCALE_LOOP
    CVB, PY, gx, gy, nz = EC.se_scale_geo(Cl, "bf16", Bl, Hl * Wl, True)
    assert (CVB, gx, gy, nz) == (32, 2, 13, 29) and nz < Bl


def act_bwd32(act, t):
    """act_bwd of csrc/dyk_common.h in fp32"""
    one, zero = torch.ones_like(t), torch.zeros_like(t)
    if act == "leaky":
        return torch.where(t > 0, one, torch.full_like(t, 0.1))
    if act == "relu":
        return torch.where(t > 0, one, zero)
    if act == "relu6":
        return torch.where((t > 0) & (t < 6), one, zero)
    if act == "hard-swish":
        return torch.where(t < -3, zero, torch.where(t <= 3, t * torch.tensor(1.0 / 3.0) + 0.5, one))
    if act == "mish":
        e = torch.exp(t.clamp(max=20.0))
        n = e * (e + 2.0)
        d = n + 2.0
        return (n * d + (4.0 * t) * (e * e + e)) * (1.0 / (d * d))
    return one


@pytest.mark.parametrize("act", O.REDUCE_ACTS)
@pytest.mark.parametrize("dt,C", [("bf16", 8), ("f32", 4)])
def test_se_scale_reduce_emulation_and_mutants(dt, C, act):
    """sums formed in fp32, pixel after pixel, from the STORED gradient stay inside the bound at the smallest chain length the launch
    geometry gives; sums from the unrounded gradient (bf16), a missing rstd and S1 where S2 belongs are flagged"""
    B, H, W = 2, 33, 17
    dz, yraw, old, p0, p1, vecs = EC.se_reduce_problem(B, C, H, W, dt)
    x32 = dz * p0[:, :, None, None] + (p1 * torch.tensor(1.0 / (H * W)))[:, :, None, None]
    g = O.store(x32, EC.DTYPES[dt]).float()
    v = lambda i: vecs[i].view(1, -1, 1, 1)

    def sums(grad, rstd=True, swap=False):
        da = grad * act_bwd32(act, yraw * v(0) + v(1))
        xh = (yraw - v(2)) * (v(3) if rstd else 1.0)
        s1, s2 = torch.zeros(C), torch.zeros(C)
        for b in range(B):
            for p in range(H * W):
                s1 = s1 + da[b, :, p // W, p % W]
                s2 = s2 + (da * xh)[b, :, p // W, p % W]
        return torch.stack([s1, s1] if swap else [s1, s2])
    m = EC.se_reduce_m(C, dt, B, H * W)
    S, b = O.se_reduce(g, yraw, vecs, act, m)
    case = "33x17 c%d %s" % (C, act)
    # (the emulation's chain is B * H * W long, the kernel's m: the bound for the emulation is taken at its own length)
    Se, be = O.se_reduce(g, yraw, vecs, act, B * H * W)
    _report("se_scale-reduce-" + dt, *O.check(sums(g), Se, be), case)
    assert m < B * H * W and bool((b <= be).all())
    fine = sums(g).double()                                   # a kernel inside the bound, to which each mutant's error is added
    if dt == "bf16":
        _flagged(O.check(fine + (sums(x32) - sums(g)).double(), S, b)[1], "sums from the unrounded gradient", case)
    _flagged(O.check(fine + (sums(g, rstd=False) - sums(g)).double(), S, b)[1], "xhat without rstd", case)
    _flagged(O.check(sums(g, swap=True), S, b)[1], "S1 where S2 belongs", case)


# ---------------------------------------------------------------------------------------------------- head
def head_bias32(dp, old, tail=True):
    """head_bias_grad_kernel: lane r takes cells r, r + 1024, r + 2048, r + 3072 into four sums while r + 3072 < cells, then single cells
    into the first; image after image; (s0 + s1) + (s2 + s3), the wave fold, the 16 wave sums in turn, the +="""
    B, na, ny, nx, no = dp.shape
    cells = ny * nx
    d = dp.permute(1, 4, 0, 2, 3).reshape(na * no, B, cells)
    s = torch.zeros(4, na * no, 1024)
    lanes = torch.arange(1024)
    for b in range(B):
        r = 0
        while r + 3072 < cells:                                           # (lane l is at r + l: live while r + l + 3072 < cells)
            for q in range(4):
                idx = r + lanes + 1024 * q
                live = (r + lanes + 3072) < cells
                s[q] = s[q] + torch.where(live, d[:, b, idx.clamp(max=cells - 1)], torch.zeros(()))
            r += 4096
        if tail:
            # lanes that left the four-load loop at trip t continue with single loads from r_l = l + 4096 t_l
            trips = torch.clamp((cells - 3072 - lanes + 4095) // 4096, min=0)
            pos = lanes + 4096 * trips
            while bool((pos < cells).any()):
                live = pos < cells
                s[0] = s[0] + torch.where(live, d[:, b, pos.clamp(max=cells - 1)], torch.zeros(()))
                pos = pos + 1024
    t = ((s[0] + s[1]) + (s[2] + s[3])).view(-1, 16, 64)
    o = 32
    while o:
        t = t[..., :o] + t[..., o:]
        o //= 2
    t = t[..., 0]
    acc = torch.zeros(na * no)
    for w in range(16):
        acc = acc + t[:, w]
    return old + acc


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ny,nx", EC.HEAD_MAPS)
def test_head_reference_and_emulation(ny, nx, B):
    na, no = EC.HEAD_NA, EC.HEAD_NO
    g = torch.Generator().manual_seed(ny * nx + B)
    dp = torch.randn(B, na, ny, nx, no, generator=g)
    old = torch.randn(na * no, generator=g)
    case = "%dx%d b%d" % (ny, nx, B)
    y = torch.randn(B, ny, nx, 24, generator=g)
    p = O.head_fwd(y[..., :18].contiguous(), na, no)
    assert torch.equal(p, y[..., :18].reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4))
    dy = O.head_bwd(dp, 24, torch.bfloat16)
    assert torch.equal(O.head_fwd(dy[..., :18].contiguous(), na, no), dp.bfloat16()) and bool((dy[..., 18:] == 0).all())
    tgt, bound = O.head_bias(dp, old)
    _report("head-bias", *O.check(head_bias32(dp, old), tgt, bound), case)
    assert torch.allclose(tgt, old.double() + O.head_bwd(dp, 18, torch.float32).double().sum((0, 1, 2)), rtol=1e-12, atol=1e-12)
    if (ny, nx) in ((5, 7), (1, 4097)):
        _flagged(O.check(head_bias32(dp, old, tail=False), tgt, bound)[1], "bias gradient skipping the tail loop", case)
    if (ny, nx) == (5, 7):
        left = torch.full((B, ny, nx, 24), EC.SENTINEL, dtype=torch.bfloat16)
        left[..., :18] = dy[..., :18]
        _flagged(O.same_bits(left, dy), "permute backward leaving pad channels unwritten", case + " ld24")
    assert (EC.head_main_trips(ny * nx) > 0) == (ny * nx > 3072)


# ---------------------------------------------------------------------------------------------------- the cases reach their paths
def test_pool_paths():
    seen_k = set()
    for (H, W, k) in EC.tile_matrix():
        vs = EC.tile_variants(H, W, k)
        assert {(dt, C) for dt, C, B, lay in vs} == {(dt, C) for dt, cs in EC.TILE_C.items() for C in cs}
        assert {lay for dt, C, B, lay in vs} == {"tight", "slice"}
    assert EC.tile_threads(32 * 32) == 1024 and 32 * 32 * 64 == 65536 and EC.tile_threads(1) == 64 and EC.tile_threads(63 + 2) == 128
    assert int(EC.pool_ref(3, 8, 2, 3, 15, 1)[1].max()) <= 224 and not EC.tile_ok(3, 1, 33, 32, 8)
    for k in EC.GENERIC_KS:
        seen_k.add(EC.pool_K(k))
    for k, s in EC.STRIDED:
        assert not EC.tile_ok(k, s, 7, 9, 8)
        seen_k.add(EC.pool_K(k))
    assert seen_k == {0, 2, 3, 5, 9, 13}
    # windows outside the map on every side, and the largest code a uint8 must hold
    x = torch.zeros(1, 1, 2, 3)
    x[0, 0, 1, 2] = 1.0
    assert int(O.pool_fwd(x, 15, 1)[1].max()) == 8 * 15 + 9 and int(O.pool_fwd(torch.zeros(1, 1, 1, 1).fill_(1.0).expand(1, 1, 1, 1), 15, 1)[1].max()) == 7 * 15 + 7
    big = torch.zeros(1, 1, 16, 20)
    big[0, 0, 15, 19] = 1.0
    assert int(O.pool_fwd(big, 15, 1)[1].max()) == 224
    for (H, W) in (EC.BIG_POOL, EC.BIG_UP_BWD, EC.BIG_AXPBY):
        assert EC.ew_grid(H * W) == 4096 and H * W > EC.EW_CAP
    assert 4 * EC.BIG_UP_FWD[0] * EC.BIG_UP_FWD[1] > EC.EW_CAP
    v = EC.BIG_DOT[0] * EC.BIG_DOT[1]
    assert EC.dot_grid(v) == 1024 and EC.dot_trips(v) == 9 and EC.dot_trips(1024 * 2048) == 8 and math.ceil(30 * 3 / 2048) == EC.dot_grid(90)


def test_se_scale_paths():
    for dt, C in EC.SE_SCALE_C:
        for (H, W) in EC.SE_SCALE_MAPS:
            CVB, PY, gx, gy, nz = EC.se_scale_geo(C, dt, 2, H * W, False)
            assert CVB * PY == 256 and gx * CVB * EC.epv(dt) >= C and nz == 2
    assert EC.se_scale_geo(264, "bf16", 2, 33 * 17, False)[:4] == (32, 8, 2, 9)           # two channel groups, the second one lane wide
    assert EC.se_scale_geo(72, "bf16", 2, 15, False)[0] == 16 and EC.se_scale_geo(8, "bf16", 2, 1, False)[:2] == (1, 256)
