"""oracle/bn_act.py, the fp64 reference of csrc/bn_act.hip and its derived per-element bounds (no GPU), at the cases
tests/test_gpu_bn_act_elements.py runs on the GPU (tests/bn_act_cases.py):
  * the shapes reach the launch geometry they are named for; the activation tables are torch's functions and derivatives in float64,
    the kink conventions torch's;
  * emulations of each kernel's arithmetic written in torch (fp64 folds in the kernels' two orders, fp32 elementwise arithmetic with
    products FMA-contracted and not, the exponential off by one ulp either way, the per-thread chains and the LDS fold of the reduce)
    stay inside every bound on every small case -- each prints `BNEMU <what> <largest error / bound> <case>`;
  * the bounds are not vacuous: each of eighteen wrong kernels is flagged by a named case;
  * the share of elements within e_t of a derivative kink is at most 0.1 % on every random case and 0 on the large fields."""
import pytest
import torch
import torch.nn.functional as F

import bn_act_cases as BC
from oracle import bn_act as O

_F64 = torch.float64
SENT = BC.SENTINEL


def _report(what, ratio, bad, case):
    print("BNEMU %s %.5f %s" % (what, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s: %d elements outside their bound, largest error / bound %.3f" % (what, case, bad, ratio)


# ---------------------------------------------------------------------------------------------------- fp32 building blocks
def mul_add(x, a, b, fma):
    """x a + b in fp32: one rounding (contracted) or two"""
    return (x.double() * a.double() + b.double()).float() if fma else x * a + b


def _exp32(t, exp_ulp):
    e = torch.exp(t.clamp(max=20.0))
    if exp_ulp:
        e = torch.nextafter(e, torch.full_like(e, float("inf") * exp_ulp))
    return e


def act32(name, t, exp_ulp=0, leaky=0.1):
    """act_fwd, in fp32"""
    if name == "leaky":
        return torch.where(t > 0, t, torch.tensor(leaky, dtype=torch.float32) * t)
    if name == "mish":
        e = _exp32(t, exp_ulp)
        n = e * (e + 2.0)
        return t * (n * (1.0 / (n + 2.0)))
    if name == "relu":
        return t.clamp(min=0.0)
    if name == "relu6":
        return t.clamp(0.0, 6.0)
    if name == "hard-sigmoid":
        return (t + 3.0).clamp(0.0, 6.0) * torch.tensor(1.0 / 6.0)
    if name == "hard-swish":
        return t * (t + 3.0).clamp(0.0, 6.0) * torch.tensor(1.0 / 6.0)
    return t


def dact32(name, t, exp_ulp=0, fma=False, mutant=None):
    """act_bwd, in fp32"""
    one, zero = torch.ones_like(t), torch.zeros_like(t)
    if name == "leaky":
        return torch.where(t > 0, one, torch.full_like(t, 0.1))
    if name == "mish":
        e = _exp32(t, exp_ulp)
        n = e * (e + 2.0)
        d = n + 2.0
        num = mul_add(4.0 * t, e * e + e, n * d, fma)
        return num * (1.0 / (d * d))
    if name == "relu":
        return torch.where(t > 0, one, zero)
    if name == "relu6":
        hi = (t <= 6) if mutant == "relu6 derivative 1 at 6" else (t < 6)
        return torch.where((t > 0) & hi, one, zero)
    if name == "hard-sigmoid":
        return torch.where((t > -3) & (t < 3), torch.full_like(t, 1.0 / 6.0), zero)
    if name == "hard-swish":
        lo = (t <= -3) if mutant == "hard-swish derivative 0 at -3" else (t < -3)
        return torch.where(lo, zero, torch.where(t <= 3, mul_add(t, torch.tensor(1.0 / 3.0), torch.tensor(0.5), fma), one))
    return one


def _skip_mask(P, C, dt, mutant):
    """elements a kernel with a broken loop bound never reaches"""
    g = O.ew_grid(C, P, dt)
    m = torch.zeros(P, C, dtype=torch.bool)
    if mutant == "tail vector of the second channel group skipped" and g.gx == 2:
        m[:, (g.CV - 1) * O.epv(dt):] = True
    if mutant == "last pixel of a chunk skipped":
        ends = [min(P, (b + 1) * g.chunk) - 1 for b in range(g.live)]
        m[ends] = True
    return m


# ---------------------------------------------------------------------------------------------------- emulations of the kernels
def fold_lanes(col):
    """bn_finalize_kernel / bn_bwd_params_kernel: lane r sums replicas r, r + 32, ...; a 5-step xor-shuffle folds the lanes.  col [slots, C]"""
    lanes = torch.zeros(32, col.shape[1], dtype=_F64)
    for r in range(col.shape[0]):
        lanes[r % 32] = lanes[r % 32] + col[r]
    idx = torch.arange(32)
    for o in (16, 8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def fold_batches(col, first, second, nacc, drop_last=False):
    """the fused kernels' fold: batches of `first`, then of `second`, then singles, into nacc accumulators (u % nacc), summed as a tree"""
    slots, C = col.shape
    acc = torch.zeros(nacc, C, dtype=_F64)
    r = 0
    while r + first <= slots:
        for u in range(first - (1 if drop_last else 0)):
            acc[u % nacc] = acc[u % nacc] + col[r + u]
        r += first
    while r + second <= slots:
        for u in range(second):
            acc[u] = acc[u] + col[r + u]
        r += second
    while r < slots:
        acc[0] = acc[0] + col[r]
        r += 1
    while acc.shape[0] > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def emu_finalize(p, order, mutant=None, gamma=True, beta=True):
    """{scale, shift, mean, rstd, running_mean, running_var} as fp32, by the kernels' expressions"""
    st = p.stats
    if order == "lanes":
        s1, s2 = fold_lanes(st[:, 0]), fold_lanes(st[:, 1])
    else:
        drop = mutant == "last replica of a batch not folded"
        s1, s2 = fold_batches(st[:, 0], 16, 4, 4, drop), fold_batches(st[:, 1], 16, 4, 4, drop)
    n = float(p.count)
    mean = s1 / n
    msq = mean.float().double() ** 2 if mutant == "mean rounded to fp32 before it is squared" else mean * mean
    var = s2 / n - msq
    if mutant != "no clamp of the variance":
        var = var.clamp(min=0.0)
    eps = 0.0 if mutant == "eps dropped" else float(torch.tensor(BC.EPS, dtype=torch.float32))
    rstd64 = 1.0 / (var + eps).sqrt()
    rstd = rstd64.float()
    g = p.gamma if gamma else torch.ones(p.C)
    b = p.beta if beta else torch.zeros(p.C)
    sc = g * rstd
    sc_used = g.double() * rstd64 if mutant == "shift formed from the unrounded scale" else sc.double()
    sh = (b.double() - mean.float().double() * sc_used).float()           # (contracted; the two-rounding form is checked as well)
    sh2 = b - mean.float() * sc
    mom = torch.tensor(BC.MOMENTUM, dtype=torch.float32)
    unb = var * n / (n - 1.0) if (n > 1 and mutant != "biased variance in running_var") else var
    return {"scale": sc, "shift": sh, "shift2": sh2, "mean": mean.float(), "rstd": rstd,
            "running_mean": (1.0 - mom) * p.rm + mom * mean.float(), "running_var": (1.0 - mom) * p.rv + mom * unb.float()}


def check_finalize(p, got, ref, label, case, report=_report):
    worst = []
    for k in ("mean", "rstd", "scale", "shift", "running_mean", "running_var"):
        worst.append(report("%s-%s" % (label, k), *O.check(got[k], *ref[k]), case))
    worst.append(report(label + "-shift2", *O.check(got["shift2"], *ref["shift"]), case))
    for k in ("shift", "shift2"):
        worst.append(report("%s-%s-given" % (label, k), *O.check(got[k], *O.shift_given(p.beta, got["mean"], got["scale"])), case))
    return worst


def emu_forward(x, sc, sh, r, act, dt, fma=False, exp_ulp=0, mutant=None):
    """the stored tensor of bn_act_fwd_kernel / the pixel loop of bn_fused_fwd_kernel; elements never reached keep the sentinel"""
    P, C = x.shape
    t = mul_add(x, sc.view(1, -1), sh.view(1, -1), fma)
    if mutant == "residual added before the activation":
        z = act32(act, t + r, exp_ulp)
    else:
        z = act32(act, t, exp_ulp, leaky=0.01 if mutant == "leaky slope 0.01" else 0.1)
        if r is not None:
            z = z + r
    out = O.store(z, BC.DTYPES[dt])
    return torch.where(_skip_mask(P, C, dt, mutant), torch.full_like(out, SENT), out)


def emu_reduce(g, y, vecs, act, dt, slots, fma=False, exp_ulp=0, mutant=None):
    """bn_act_bwd_reduce_kernel: [slots, 2, C] fp64 added to zeroed replicas"""
    P, C = y.shape
    geo = O.reduce_grid(C, P, dt)
    sc, sh, mu, rs = (v.view(1, -1) for v in vecs)
    da = g * dact32(act, mul_add(y, sc, sh, fma), exp_ulp, fma, mutant)
    xh = (y - mu) * rs
    da = torch.where(_skip_mask(P, C, dt, mutant), torch.zeros_like(da), da)
    pad = geo.gy * geo.chunk - P
    da4 = F.pad(da, (0, 0, 0, pad)).view(geo.gy, geo.rows, geo.PY, C)
    xh4 = F.pad(xh, (0, 0, 0, pad)).view(geo.gy, geo.rows, geo.PY, C)
    s1 = torch.zeros(geo.gy, geo.PY, C)
    s2 = torch.zeros(geo.gy, geo.PY, C)
    for k in range(geo.rows):
        s1 = s1 + da4[:, k]
        s2 = mul_add(da4[:, k], xh4[:, k], s2, fma)
    t1, t2 = s1[:, 0], s2[:, 0]
    for q in range(1, geo.PY):
        t1, t2 = t1 + s1[:, q], t2 + s2[:, q]
    red = torch.zeros(slots, 2, C, dtype=_F64)
    for by in range(geo.gy):
        red[by % slots, 0] += t1[by].double()
        red[by % slots, 1] += t2[by].double()
    return red


def emu_apply(g, y, vecs, act, dt, red, old=None, accum=False, route=None, fma=False, exp_ulp=0, mutant=None, dgamma=None, dbeta=None):
    """bn_act_bwd_apply_kernel: (stored dy, dgamma, dbeta).  red [slots, 2, C], or with route = (H, W, offset) the wide buffer [slots, H]"""
    P, C = y.shape
    drop = mutant == "last replica of a batch not folded"
    if route is None:
        c1, c2 = red[:, 0], red[:, 1]
    else:
        H, W, off = route
        flat = red.reshape(-1)
        rs_, so = (2 * C, C) if mutant == "replica stride 2C used where H is given" else (H, W)
        rows = torch.arange(red.shape[0]).view(-1, 1) * rs_ + off + torch.arange(C).view(1, -1)
        c1, c2 = flat[rows], flat[rows + so]
    tot = [fold_batches(c, 16, 8, 8, drop).float() for c in (c1, c2)]
    dg = db = None
    if dgamma is not None:
        a, b = (tot[0], tot[1]) if mutant == "aux and aux2 swapped" else (tot[1], tot[0])
        dg, db = dgamma + a, dbeta + b
    invn = torch.tensor(1.0) / torch.tensor(float(P - 1 if mutant == "N = npix - 1" else P))
    m1, m2 = (tot[0] * invn).view(1, -1), (tot[1] * invn).view(1, -1)
    if mutant == "m1 and m2 swapped":
        m1, m2 = m2, m1
    sc, sh, mu, rs = (v.view(1, -1) for v in vecs)
    da = g * dact32(act, mul_add(y, sc, sh, fma), exp_ulp, fma, mutant)
    xh = (y - mu) * (sc if mutant == "xhat formed with scale in place of rstd" else rs)
    inner = (da - m1).double() - xh.double() * m2.double() if fma else (da - m1) - xh * m2
    r = sc * inner.float()
    if accum and mutant != "ACCUM ignored":
        r = r + old
    out = O.store(r, BC.DTYPES[dt])
    base = old if accum else torch.full_like(out, SENT)
    return torch.where(_skip_mask(P, C, dt, mutant), O.store(base, BC.DTYPES[dt]), out), dg, db


# ---------------------------------------------------------------------------------------------------- the cases are what they claim
@pytest.mark.parametrize("sid,dt", BC.SMALL + [(BC.BIG.id, d) for d in BC.BIG.C])
def test_each_shape_reaches_its_geometry(sid, dt):
    g = BC.assert_geometry(sid, dt)
    s = BC.BY_ID[sid]
    assert g.CV * O.epv(dt) == s.C[dt] and (g.live - 1) * g.chunk + g.last == s.npix and g.rows == -(-g.chunk // g.PY)
    if sid in ("35", "577"):
        assert g.CV % g.CVB != 0                        # idle tx columns
    if sid == "577":
        assert g.CV - g.CVB == 1 and g.gy < 16          # a one-vector tail group; fewer workgroups than backward replicas
    if sid == "4099":
        assert g.gy > 16                                # the slot index wraps
    if sid == "65537":
        assert g.gy == 2048 // g.gx and g.rows > 8      # the capped grid, a third trip of the U = 4 loop


@pytest.mark.parametrize("act", BC.ACTS)
def test_activation_tables_are_torch_in_float64(act):
    fn = {"linear": lambda t: t, "leaky": lambda t: F.leaky_relu(t, 0.1), "mish": F.mish, "relu": F.relu, "relu6": F.relu6,
          "hard-sigmoid": F.hardsigmoid, "hard-swish": F.hardswish}[act]
    g = torch.Generator().manual_seed(5)
    t = torch.cat([torch.randn(4096, generator=g, dtype=_F64) * 4, torch.tensor(BC.KINK_VALUES, dtype=_F64)]).requires_grad_(True)
    z = fn(t)
    z.sum().backward()
    assert float((O.act64(act, t.detach()) - z.detach()).abs().max()) <= 1e-12
    off = torch.ones_like(t.detach(), dtype=torch.bool)         # AT a kink the convention below decides, not this torch build's CPU kernel
    for kink, _ in O._ACT_D[act][1]:
        off &= t.detach() != kink
    assert float((O._ACT_D[act][0](t.detach()) - t.grad)[off].abs().max()) <= {"leaky": 2e-9, "hard-sigmoid": 1e-8}.get(act, 1e-12)     # (the table holds 0.1f; torch's fp64 kernel 1 / 6f)
    for kink, want in BC.KINK_CONVENTION.get(act, {}).items():
        at = torch.tensor([kink], dtype=_F64)
        assert float(O._ACT_D[act][0](at)) == pytest.approx(want, abs=2e-9)
        assert float(BC.kink_da(act)[0, BC.KINK_VALUES.index(kink)]) == float(torch.tensor(want, dtype=torch.float32))
    assert act in O._ACT and set(O._ACT) == set(O._ACT_D) == set(BC.ACTS) and len(BC.ACTS) == 7


# ---------------------------------------------------------------------------------------------------- finalize / fold
FIN_CASES = [(8, 1), (24, 35), (264, 577), (72, 4099), (264, 65537)]


@pytest.mark.parametrize("slots", sorted(set(BC.FIN_SLOTS + BC.FUSED_SLOTS)))
@pytest.mark.parametrize("C,count", FIN_CASES)
def test_finalize_emulations_stay_inside_every_bound(C, count, slots):
    p = BC.fin_problem(C, count, slots)
    ref = BC.fin_ref(p)
    case = "C%d n%d slots %d" % (C, count, slots)
    for order in ("lanes", "batches"):
        check_finalize(p, emu_finalize(p, order), ref, order, case)
    q = p._replace(gamma=torch.ones(C), beta=torch.zeros(C))
    got = emu_finalize(q, "lanes")
    ref0 = BC.fin_ref(p, gamma=False, beta=False)
    for k in ("scale", "shift"):
        _report("null-" + k, *O.check(got[k], *ref0[k]), case)


@pytest.mark.parametrize("count", [35, 577, 4099, 65537])
def test_constant_channel_has_a_negative_variance_before_the_clamp(count):
    p = BC.fin_problem(24, count, 4)
    ref = BC.fin_ref(p)
    assert float(ref["raw_var"][0][p.const]) < 0.0 and float(ref["var"][0][p.const]) == 0.0
    assert float(ref["raw_var"][0][3]) < -BC.EPS and float(ref["var"][0][3]) == 0.0
    assert float(ref["scale"][0][p.zero_gamma]) == 0.0 and float(p.gamma[p.zero_gamma]) == 0.0


def test_fold_emulation_stays_inside_its_bound():
    for C in (1, 24, 264):
        g, b, rm, rv = BC.fold_problem(C)
        eps = torch.tensor(BC.EPS)
        for gg, bb in ((g, b), (None, b), (g, None), (None, None)):
            ref = O.fold(rm, rv, BC.EPS, gg, bb)
            sc = (torch.ones(C) if gg is None else gg) / (rv + eps).sqrt()
            sh = (torch.zeros(C) if bb is None else bb) - rm * sc
            _report("fold-scale", *O.check(sc, *ref["scale"]), "C%d" % C)
            _report("fold-shift", *O.check(sh, *ref["shift"]), "C%d" % C)
            bad = O.check((torch.zeros(C) if bb is None else bb) - rm * (sc * (1 + 2.0 ** -19)), *ref["shift"])[1]
            assert bad > 0 or C == 1


# ---------------------------------------------------------------------------------------------------- forward / reduce / apply
VARIANTS = [(False, 0), (True, 0), (False, 1), (True, -1)]          # (products contracted, expf off by this many ulps)


@pytest.mark.parametrize("sid,dt", BC.SMALL)
def test_forward_emulations_stay_inside_every_bound(sid, dt):
    p = BC.problem(sid, dt)
    sc, sh = p.vecs[0], p.vecs[1]
    for act in BC.ACTS:
        for res in (None, p.res):
            ref = O.forward(p.y, sc, sh, act, BC.DTYPES[dt], res)
            for fma, eu in VARIANTS if act == "mish" else VARIANTS[:2]:
                _report("fwd-%s%s" % (act, "-res" if res is not None else ""), *O.check(emu_forward(p.y, sc, sh, res, act, dt, fma, eu), *ref),
                        "%s %s fma%d exp%+d" % (sid, dt, fma, eu))
    if dt == "f16":
        big = torch.full_like(sc, 6.0e4)
        got = emu_forward(p.y, big, sh, None, "linear", dt)
        _report("fwd-saturating", *O.check(got, *O.forward(p.y, big, sh, "linear", torch.float16)), "%s f16" % sid)
        assert float(got.abs().max()) == O.F16_MAX


@pytest.mark.parametrize("sid,dt", BC.TRAIN)
def test_reduce_emulations_stay_inside_every_bound(sid, dt):
    p = BC.problem(sid, dt)
    geo = BC.geometry(sid, dt, reduce=True)
    for act in BC.ACTS:
        S, b = O.reduce(p.g, p.y, p.vecs, act, geo)
        for fma, eu in VARIANTS if act == "mish" else VARIANTS[:2]:
            for slots in BC.REDUCE_SLOTS if (act == "leaky" and not fma) else [4]:
                got = emu_reduce(p.g, p.y, p.vecs, act, dt, slots, fma, eu).sum(0)
                _report("reduce-%s" % act, *O.check(got, S, b), "%s %s fma%d exp%+d slots %d" % (sid, dt, fma, eu, slots))


@pytest.mark.parametrize("sid,dt", BC.TRAIN)
def test_apply_emulations_stay_inside_every_bound(sid, dt):
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        slots = BC.APPLY_SLOTS[i % len(BC.APPLY_SLOTS)]
        red = BC.replicas(p.C, slots, p.P)
        S, e_fold = O.totals(red)
        for accum in (False, True):
            ref = O.apply(p.g, p.y, p.vecs, act, S, p.P, BC.DTYPES[dt], p.old if accum else None)
            for fma, eu in VARIANTS if act == "mish" else VARIANTS[:2]:
                got, dg, db = emu_apply(p.g, p.y, p.vecs, act, dt, red, p.old, accum, None, fma, eu, None, torch.ones(p.C), -torch.ones(p.C))
                case = "%s %s slots %d accum%d fma%d exp%+d" % (sid, dt, slots, accum, fma, eu)
                _report("apply-%s" % act, *O.check(got, *ref), case)
                _report("apply-dgamma", *O.check(dg, *O.param_bound(S[1], e_fold[1], torch.ones(p.C))), case)
                _report("apply-dbeta", *O.check(db, *O.param_bound(S[0], e_fold[0], -torch.ones(p.C))), case)
    wide, H, W, off = BC.route_red(BC.replicas(p.C, 16, p.P))
    S, _ = O.totals(BC.replicas(p.C, 16, p.P))
    got = emu_apply(p.g, p.y, p.vecs, "leaky", dt, wide, route=(H, W, off))[0]
    _report("apply-route", *O.check(got, *O.apply(p.g, p.y, p.vecs, "leaky", S, p.P, BC.DTYPES[dt])), "%s %s" % (sid, dt))


def test_kink_field_is_exact_and_follows_the_convention():
    y, g, vecs = BC.kink_field()
    for act in BC.ACTS:
        r = O.dact(g, y, vecs[0], vecs[1], act)
        assert float(r.e_t.max()) == 0.0 and not bool(r.near.any()) and torch.equal(r.t, y.double())
        if act != "mish":
            for fma in (False, True):
                got = dact32(act, y, fma=fma)
                m = (y.abs() >= 3) | (act != "hard-swish")
                assert torch.equal(got[m], BC.kink_da(act)[m]), act
                assert O.check(got, r.da, r.e_da)[1] == 0


# ---------------------------------------------------------------------------------------------------- wrong kernels
def _flag_finalize(mutant, C, count, slots, keys, order="lanes"):
    p = BC.fin_problem(C, count, slots)
    ref, got = BC.fin_ref(p), emu_finalize(p, order, mutant)
    bad = sum(O.check(got[k], *ref[k])[1] for k in keys if k != "given")
    if "given" in keys:
        bad += O.check(got["shift"], *O.shift_given(p.beta, got["mean"], got["scale"]))[1]
    return bad


def _flag_forward(mutant, sid, dt, act):
    p = BC.problem(sid, dt)
    got = emu_forward(p.y, p.vecs[0], p.vecs[1], p.res, act, dt, mutant=mutant)
    return O.check(got, *O.forward(p.y, p.vecs[0], p.vecs[1], act, BC.DTYPES[dt], p.res))[1]


def _flag_kink(mutant, act):
    y, g, vecs = BC.kink_field()
    red = emu_reduce(g, y, vecs, act, "bf16", 1, mutant=mutant)
    dy = emu_apply(g, y, vecs, act, "bf16", torch.zeros(1, 2, 16, dtype=_F64), mutant=mutant)[0]
    S, b = O.reduce(g, y, vecs, act, O.reduce_grid(16, 1, "bf16"))
    want = BC.kink_da(act)
    return O.check(red.sum(0), S, b)[1] + int((red[0, 0].float() != want[0]).sum()) + O.same_bits(dy, want.bfloat16())


def _flag_apply(mutant, sid, dt, act="leaky", slots=16, accum=False, route=False, params=False):
    p = BC.problem(sid, dt)
    red = BC.replicas(p.C, slots, p.P)
    S, e_fold = O.totals(red)
    src, rt = red, None
    if route:
        src, H, W, off = BC.route_red(red)
        rt = (H, W, off)
    got, dg, db = emu_apply(p.g, p.y, p.vecs, act, dt, src, p.old, accum, rt, mutant=mutant, dgamma=torch.ones(p.C), dbeta=torch.ones(p.C))
    if params:
        return O.check(dg, *O.param_bound(S[1], e_fold[1], torch.ones(p.C)))[1] + O.check(db, *O.param_bound(S[0], e_fold[0], torch.ones(p.C)))[1]
    return O.check(got, *O.apply(p.g, p.y, p.vecs, act, S, p.P, BC.DTYPES[dt], p.old if accum else None))[1]


def _flag_reduce(mutant, sid, dt, act="leaky"):
    p = BC.problem(sid, dt)
    S, b = O.reduce(p.g, p.y, p.vecs, act, BC.geometry(sid, dt, True))
    return O.check(emu_reduce(p.g, p.y, p.vecs, act, dt, 4, mutant=mutant).sum(0), S, b)[1]


WRONG = {
    "biased variance in running_var": lambda m: _flag_finalize(m, 264, 65537, 4, ["running_var"]),
    "eps dropped": lambda m: _flag_finalize(m, 24, 35, 4, ["rstd", "scale"]),
    "no clamp of the variance": lambda m: _flag_finalize(m, 24, 577, 4, ["running_var", "rstd"]),
    "mean rounded to fp32 before it is squared": lambda m: _flag_finalize(m, 24, 35, 1, ["rstd"]),
    "shift formed from the unrounded scale": lambda m: _flag_finalize(m, 264, 577, 4, ["given"]),
    "residual added before the activation": lambda m: _flag_forward(m, "35", "f32", "relu"),
    "leaky slope 0.01": lambda m: _flag_forward(m, "35", "bf16", "leaky"),
    "relu6 derivative 1 at 6": lambda m: _flag_kink(m, "relu6"),
    "hard-swish derivative 0 at -3": lambda m: _flag_kink(m, "hard-swish"),
    "m1 and m2 swapped": lambda m: _flag_apply(m, "35", "f32"),
    "xhat formed with scale in place of rstd": lambda m: _flag_apply(m, "35", "bf16"),
    "aux and aux2 swapped": lambda m: _flag_apply(m, "1", "bf16", params=True),
    "last replica of a batch not folded": lambda m: _flag_apply(m, "35", "bf16", slots=16) * _flag_apply(m, "35", "bf16", slots=31)
    * _flag_finalize(m, 24, 35, 23, ["mean"], "batches"),
    "replica stride 2C used where H is given": lambda m: _flag_apply(m, "35", "bf16", route=True),
    "ACCUM ignored": lambda m: _flag_apply(m, "35", "bf16", accum=True),
    "N = npix - 1": lambda m: _flag_apply(m, "4099", "bf16"),
    "tail vector of the second channel group skipped": lambda m: _flag_forward(m, "577", "bf16", "leaky") * _flag_apply(m, "577", "f32")
    * _flag_reduce(m, "577", "bf16"),
    "last pixel of a chunk skipped": lambda m: _flag_forward(m, "577", "f32", "leaky") * _flag_apply(m, "4099", "bf16") * _flag_reduce(m, "2049", "bf16"),
}


@pytest.mark.parametrize("mutant", list(WRONG))
def test_wrong_kernel_is_flagged(mutant):
    bad = WRONG[mutant](mutant)
    print("BNWRONG %s: %d elements outside their bound" % (mutant, bad))
    assert bad > 0, "%s is NOT flagged" % mutant


def test_the_unmutated_emulations_pass_where_the_wrong_kernels_are_flagged():
    """the same calls with no mutation: nothing is flagged, so the flags above are the mutations' doing"""
    for name, fn in WRONG.items():
        assert fn(None) == 0, name


# ---------------------------------------------------------------------------------------------------- kinks
@pytest.mark.parametrize("sid,dt", BC.TRAIN + [(BC.BIG.id, "bf16")])
def test_share_of_elements_at_a_derivative_kink(sid, dt):
    p = BC.problem(sid, dt)
    for act in ("leaky", "relu6", "hard-swish", "hard-sigmoid") if sid != BC.BIG.id else ("leaky",):
        share = O.kink_share(p.y, p.vecs[0], p.vecs[1], act)
        print("BNKINK %s %s %s %.3g" % (sid, dt, act, share))
        assert share <= O.KINK_SHARE
        if (sid, dt) in (("577", "bf16"), ("577", "f32"), ("4099", "bf16"), (BC.BIG.id, "bf16")):
            assert share == 0.0
