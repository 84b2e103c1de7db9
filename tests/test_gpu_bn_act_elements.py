"""csrc/bn_act.hip held to the fp64 reference of oracle/bn_act.py, element by element, on every path of its seven entry points.

Every launch writes into buffers pre-filled with a sentinel: rows that are tight or the channel slice [EPV : EPV + C] of rows of
C + 3 EPV elements (chosen independently for a, b and out), between guard rows; parameter vectors, statistics replicas, dgamma / dbeta
between sentinel frames.  Afterwards inputs, guards, padding and every replica the kernel must not write are bit-identical and every
element in range is inside its derived bound (tests/test_bn_act_reference.py shows on the CPU that the bounds admit emulations of the
kernels' arithmetic and flag eighteen kinds of wrong kernel).  The cases are those of tests/bn_act_cases.py; each shape asserts the launch
geometry it is named for.

Kernel instantiations bn_act.hip launches, and a case that reaches each:
  dyk_bn_finalize           bn_finalize_kernel: test_finalize (1 .. 256 replicas: lanes r, r + 32, ...; count == 1; the constant channels;
                            null gamma / beta / running / save), gridDim.z = 2 in test_twin_launches
  dyk_bn_fold               bn_fold_kernel: test_fold (C = 1, 24, 264: two workgroups; null gamma, null beta)
  dyk_bn_act_fwd            bn_act_fwd_kernel<bf16 | f16 | float, ACT> for the seven ACT: test_forward at every small shape (f16 at 1, 35
                            and 577 pixels, with the saturating store); <bf16 | float, leaky> at 65537 pixels in test_forward_capped_grid
  dyk_bn_finalize_act_fwd   bn_fused_fwd_kernel<bf16 | float, ACT> for the seven ACT: test_fused_forward (1 .. 32 replicas: batches of 16
                            and 4 plus singles); <bf16, leaky> at 65537 pixels in test_fused_forward_capped_grid
  dyk_bn_act_bwd_reduce     bn_act_bwd_reduce_kernel<bf16 | float, ACT> for the seven ACT: test_reduce (1, 4, 16 replicas; gy = 33 wraps
                            the slot index, gy = 10 leaves replicas untouched), test_kink_field; <bf16, leaky> in test_reduce_capped_grid
  dyk_bn_bwd_params         bn_bwd_params_kernel: test_params (1 .. 256 replicas, null dgamma / dbeta)
  dyk_bn_act_bwd_apply      bn_act_bwd_apply_kernel<bf16 | float, ACT> for the seven ACT: test_apply (1 .. 31 replicas: batches of 16 and 8
                            plus singles; ACCUM; aux / aux2 null or set; the columns of a wider reduction), test_kink_field; <bf16, leaky>
                            in test_apply_capped_grid
  every kernel with gridDim.z = 2: test_twin_launches.  Refusals and DYK_EW_SKIP: test_refusals.

Every check prints `BNRATIO <what> <dtype> <largest error / bound> <case>`; DESIGN.md ("BatchNorm/activation kernels against fp64") records
the largest per operation and type."""
import ctypes

import pytest
import torch

import bn_act_cases as BC
from bn_act_cases import SENTINEL, Flat
from oracle import bn_act as O

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _L():
    from dyk import lib as L
    return L


def _lib():
    return _L().load()


def _code(dt):
    L = _L()
    return {"bf16": L.DYK_BF16, "f32": L.DYK_F32, "f16": L.DYK_F16}[dt]


def _sync_ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)
    torch.cuda.synchronize()


def _report(what, dt, ratio, bad, case):
    print("BNRATIO %s %s %.5f %s" % (what, dt, ratio, case))
    assert bad == 0 and ratio <= 1.0, "%s %s %s: %d elements outside their bound, largest error / bound %.3f" % (what, dt, case, bad, ratio)


def _out_vec(C, dtype=torch.float32):
    return Flat(torch.empty(C, dtype=dtype), fill=SENTINEL).arm()


def _bits(buf):
    return buf.t.cpu().clone()


def _lays(i):
    """row layouts of (a, b, out), chosen independently: the i-th of the eight combinations"""
    return tuple(BC.LAYOUTS[(i >> k) & 1] for k in range(3))


def _pair(call, x, y):
    """one two-problem launch of x and y"""
    x.d.twin = ctypes.addressof(y.d)
    try:
        return call(x)
    finally:
        x.d.twin = None


# ---------------------------------------------------------------------------------------------------- finalize
class Fin:
    """the operands of dyk_bn_finalize / the finalize half of dyk_bn_finalize_act_fwd, framed"""

    def __init__(self, p, gamma=True, beta=True, running=True, save=True):
        self.p, self.opts = p, (gamma, beta, running)
        self.stats = Flat(p.stats).arm()
        self.gamma = Flat(p.gamma).arm() if gamma else None
        self.beta = Flat(p.beta).arm() if beta else None
        self.rm, self.rv = (Flat(p.rm).arm(), Flat(p.rv).arm()) if running else (None, None)
        self.scale, self.shift = _out_vec(p.C), _out_vec(p.C)
        self.mean, self.rstd = (_out_vec(p.C), _out_vec(p.C)) if save else (None, None)
        d = self.d = _L().DykBnFinalizeDesc()
        ptr = lambda f: f.t.data_ptr() if f is not None else None
        d.stats, d.gamma, d.beta, d.running_mean, d.running_var = ptr(self.stats), ptr(self.gamma), ptr(self.beta), ptr(self.rm), ptr(self.rv)
        d.scale, d.shift, d.save_mean, d.save_rstd = ptr(self.scale), ptr(self.shift), ptr(self.mean), ptr(self.rstd)
        d.C, d.count, d.momentum, d.eps, d.slots = p.C, p.count, BC.MOMENTUM, BC.EPS, p.slots

    def launch(self):
        _sync_ok(_lib().dyk_bn_finalize(ctypes.byref(self.d), None), "dyk_bn_finalize")

    def verify(self, what, case, rearmed):
        p = self.p
        for f in (self.gamma, self.beta):
            if f is not None:
                f.assert_untouched()
        for f in (self.scale, self.shift, self.mean, self.rstd, self.rm, self.rv):
            if f is not None:
                f.assert_outside_untouched()
        if rearmed:
            self.stats.assert_outside_untouched()
            assert bool((self.stats.t == 0).all()), "finalize must leave its replicas exactly zero"
        else:
            self.stats.assert_untouched()
        ref = BC.fin_ref(p, *self.opts)
        got = {"scale": self.scale, "shift": self.shift, "mean": self.mean, "rstd": self.rstd, "running_mean": self.rm, "running_var": self.rv}
        for k, f in got.items():
            if f is not None:
                _report("%s-%s" % (what, k), "f32", *O.check(f.t.cpu(), *ref[k]), case)
        if self.mean is not None:
            tgt, b = O.shift_given(p.beta if self.opts[1] else None, self.mean.t.cpu(), self.scale.t.cpu())
            _report(what + "-shift-given", "f32", *O.check(self.shift.t.cpu(), tgt, b), case)
        return [f.t.cpu().clone() for f in got.values() if f is not None]


FIN_CASES = [(8, 1), (24, 35), (264, 577), (264, 65537)]


@pytest.mark.parametrize("C,count", FIN_CASES)
def test_finalize(C, count):
    """every replica count (more than 32: lanes r, r + 32, ...), count == 1, the constant channels whose fp64 variance is negative before the
    clamp, gamma == 0; null gamma / beta / running_* / save_*; the replicas are exactly zero afterwards"""
    for slots in BC.FIN_SLOTS:
        f = Fin(BC.fin_problem(C, count, slots))
        f.launch()
        f.verify("finalize", "C%d n%d slots %d" % (C, count, slots), rearmed=True)
    for i, opts in enumerate(((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                              (False, False, False, False))):
        f = Fin(BC.fin_problem(C, count, BC.FIN_SLOTS[i]), *opts)
        f.launch()
        f.verify("finalize-null", "C%d n%d gamma%d beta%d running%d save%d" % ((C, count) + opts), rearmed=True)


def test_fold():
    for C in (1, 24, 264):
        g, b, rm, rv = BC.fold_problem(C)
        for gg, bb in ((g, b), (None, b), (g, None), (None, None)):
            ins = [Flat(v).arm() if v is not None else None for v in (gg, bb, rm, rv)]
            sc, sh = _out_vec(C), _out_vec(C)
            ptr = [f.t.data_ptr() if f is not None else None for f in ins]
            _sync_ok(_lib().dyk_bn_fold(ptr[0], ptr[1], ptr[2], ptr[3], BC.EPS, sc.t.data_ptr(), sh.t.data_ptr(), C, None), "dyk_bn_fold")
            for f in ins:
                if f is not None:
                    f.assert_untouched()
            ref = O.fold(rm, rv, BC.EPS, gg, bb)
            case = "C%d gamma%d beta%d" % (C, gg is not None, bb is not None)
            for k, f in (("scale", sc), ("shift", sh)):
                f.assert_outside_untouched()
                _report("fold-" + k, "f32", *O.check(f.t.cpu(), *ref[k]), case)
    assert _lib().dyk_bn_fold(None, None, None, ptr[3], BC.EPS, sc.t.data_ptr(), sh.t.data_ptr(), C, None) == ERR_ARG
    assert _lib().dyk_bn_fold(None, None, ptr[2], ptr[3], BC.EPS, sc.t.data_ptr(), sh.t.data_ptr(), 0, None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------- forward
class Fwd:
    """one forward problem: z = act(x sc + sh) (+ r).  alt: a second, different problem of the same shape (for the two-problem launch)"""

    def __init__(self, p, act, lays=("tight", "tight", "tight"), res=True, alt=False, params=True, scale=None, inplace=False, fin=None):
        self.p, self.act, self.fin, self.inplace = p, act, fin, inplace
        self.x, r = (p.g, p.old) if alt else (p.y, p.res)
        self.r = r if res else None
        sc, sh = (p.vecs[3], p.vecs[2]) if alt else (p.vecs[0] if scale is None else scale, p.vecs[1])
        self.sc, self.sh = (sc, sh) if params and fin is None else (None, None)
        self.a = BC.rows_buf(p.P, p.C, p.dt, lays[0], self.x)
        self.b = BC.rows_buf(p.P, p.C, p.dt, lays[1], self.r) if res else None
        self.o = self.a if inplace else BC.rows_buf(p.P, p.C, p.dt, lays[2])
        self.fsc, self.fsh = (Flat(sc).arm(), Flat(sh).arm()) if self.sc is not None else (None, None)
        d = self.d = _L().DykEwDesc()
        d.a, d.out, d.lda, d.ldo = self.a.t.data_ptr(), self.o.t.data_ptr(), self.a.ld, self.o.ld
        if res:
            d.b, d.ldb = self.b.t.data_ptr(), self.b.ld
        if self.fsc is not None:
            d.p0, d.p1 = self.fsc.t.data_ptr(), self.fsh.t.data_ptr()
        d.dtype, d.npix, d.C, d.act = _code(p.dt), p.P, p.C, _L().ACT_CODES[act]

    def launch(self):
        if self.fin is not None:
            _sync_ok(_lib().dyk_bn_finalize_act_fwd(ctypes.byref(self.fin.d), ctypes.byref(self.d), None), "dyk_bn_finalize_act_fwd")
        else:
            _sync_ok(_lib().dyk_bn_act_fwd(ctypes.byref(self.d), None), "dyk_bn_act_fwd")

    def verify(self, what, case):
        p = self.p
        for f in (self.b, self.fsc, self.fsh) + (() if self.inplace else (self.a,)):
            if f is not None:
                f.assert_untouched()
        self.o.assert_outside_untouched()
        sc, sh = self.sc, self.sh
        if self.fin is not None:                     # held to the scale / shift the launch itself published
            sc, sh = self.fin.scale.t.cpu(), self.fin.shift.t.cpu()
        _report(what, p.dt, *O.check(BC.get_rows(self.o), *O.forward(self.x, sc, sh, self.act, BC.DTYPES[p.dt], self.r)), case)
        return _bits(self.o)


@pytest.mark.parametrize("sid,dt", BC.SMALL)
def test_forward(sid, dt):
    """the seven activations with and without the residual over the eight (a, b, out) layout combinations; null scale / shift; the in-place
    form; fp16's saturating store"""
    BC.assert_geometry(sid, dt)
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        for res in (True, False):
            lays = _lays(i + 4 * res)
            f = Fwd(p, act, lays, res)
            f.launch()
            want = f.verify("fwd-" + act, "%s %s res%d" % (sid, "/".join(lays), res))
            if i % 3 == 0:
                g = Fwd(p, act, lays, res, inplace=True)
                g.launch()
                assert torch.equal(g.verify("fwd-inplace-" + act, sid), want), "the in-place form differs from the out-of-place one"
    for act in ("relu", "linear") if dt == "f32" else ("leaky", "mish"):
        f = Fwd(p, act, _lays(5), True, params=False)
        f.launch()
        f.verify("fwd-null-params-" + act, sid)
    if dt == "f16":
        f = Fwd(p, "linear", _lays(2), False, scale=torch.full((p.C,), 6.0e4))
        f.launch()
        f.verify("fwd-saturating", sid)
        assert float(BC.get_rows(f.o).abs().max()) == O.F16_MAX, "no result saturated"


@pytest.mark.parametrize("dt", list(BC.BIG.C))
def test_forward_capped_grid(dt):
    """65537 pixels: gy capped at 1024, nine rows per thread (a third, partial trip of the U = 4 loop), 113 workgroups with an empty chunk"""
    BC.assert_geometry(BC.BIG.id, dt)
    f = Fwd(BC.problem(BC.BIG.id, dt), "leaky", ("tight", "slice", "slice"), True)
    f.launch()
    f.verify("fwd-leaky", BC.BIG.id)


def _fused(p, act, slots, lays, res, opts=(True, True, True, True)):
    fin = Fin(BC.fin_problem(p.C, p.P, slots), *opts)
    if fin.p.const is not None and p.dt == "f32":       # the constant channel of the statistics is constant in the tensor too
        y = p.y.clone()
        y[:, fin.p.const] = BC.const_stats(p.P, slots)[0]
        p = p._replace(y=y)
    f = Fwd(p, act, lays, res, fin=fin)
    f.launch()
    case = "%s %s slots %d %s" % (p.sid, act, slots, "/".join(lays))
    fin.verify("fused", case, rearmed=False)           # replicas bit-identical; running statistics inside the bound of ONE blend
    f.verify("fused-fwd-" + act, case)
    return f, fin


@pytest.mark.parametrize("sid,dt", BC.TRAIN)
def test_fused_forward(sid, dt):
    """dyk_bn_finalize_act_fwd: every replica count of the fold (16 + 4 + singles) with an activation each; the statistics are published by
    grid row 0 only (gy > 1 at 2049, 4099, 577 pixels: one blend of the running statistics) and the replicas stay as they were"""
    g = BC.assert_geometry(sid, dt)
    p = BC.problem(sid, dt)
    for i, (act, slots) in enumerate(zip(BC.ACTS, BC.FUSED_SLOTS)):
        _fused(p, act, slots, _lays(i), bool(i & 1))
    _fused(p, "leaky", 23 if g.gy > 1 else 7, _lays(6), True, (False, False, False, False))


def test_fused_forward_capped_grid():
    BC.assert_geometry(BC.BIG.id, "bf16")
    _fused(BC.problem(BC.BIG.id, "bf16"), "leaky", 32, ("slice", "tight", "tight"), True)


# ---------------------------------------------------------------------------------------------------- backward
def _alt(p):
    """a second, different problem of the same shape"""
    return p._replace(y=p.res, g=p.old, res=p.y, old=p.g, vecs=p.vecs[[0, 1, 3, 2]].flip(1).contiguous())


class Bwd:
    """the operands of the reduce and the apply: a = dz, b = yraw, four vectors, replicas [slots, 2, C] (or columns of a wider buffer)"""

    def __init__(self, p, act, lays=("tight", "tight", "tight"), red=None, slots=1, route=False, accum=False, aux=True, inplace=False, out=True):
        self.p, self.act, self.accum, self.inplace, self.slots = p, act, accum, inplace, slots
        self.a = BC.rows_buf(p.P, p.C, p.dt, lays[0], p.g)
        self.b = BC.rows_buf(p.P, p.C, p.dt, lays[1], p.y)
        self.o = None
        if out:
            self.o = self.a if inplace else BC.rows_buf(p.P, p.C, p.dt, lays[2], p.old if accum else None)
        self.vecs = Flat(p.vecs).arm()
        self.red_h = torch.zeros(slots, 2, p.C, dtype=torch.float64) if red is None else red
        d = self.d = _L().DykEwDesc()
        if route:
            wide, d.H, d.W, off = BC.route_red(self.red_h)
            self.red = Flat(wide).arm()
            d.red = self.red.t.data_ptr() + 8 * off
        else:
            self.red = Flat(self.red_h).arm()
            d.red = self.red.t.data_ptr()
        self.dg, self.db = (Flat(torch.full((p.C,), 0.25)).arm(), Flat(torch.full((p.C,), -0.5)).arm()) if aux else (None, None)
        d.a, d.b, d.lda, d.ldb = self.a.t.data_ptr(), self.b.t.data_ptr(), self.a.ld, self.b.ld
        if out:
            d.out, d.ldo = self.o.t.data_ptr(), self.o.ld
        d.p0, d.p1, d.p2, d.p3 = (self.vecs.t[i].data_ptr() for i in range(4))
        if aux:
            d.aux, d.aux2 = self.dg.t.data_ptr(), self.db.t.data_ptr()
        d.dtype, d.npix, d.C, d.act, d.slots = _code(p.dt), p.P, p.C, _L().ACT_CODES[act], slots
        d.flags = _L().EW_ACCUM if accum else 0

    def reduce(self):
        _sync_ok(_lib().dyk_bn_act_bwd_reduce(ctypes.byref(self.d), None), "dyk_bn_act_bwd_reduce")

    def apply(self):
        _sync_ok(_lib().dyk_bn_act_bwd_apply(ctypes.byref(self.d), None), "dyk_bn_act_bwd_apply")

    def inputs_untouched(self):
        for f in (self.b, self.vecs) + (() if self.inplace else (self.a,)):
            f.assert_untouched()

    def verify_reduce(self, what, case):
        p = self.p
        self.inputs_untouched()
        self.red.assert_outside_untouched()
        geo = O.reduce_grid(p.C, p.P, p.dt)
        got = self.red.t.cpu()
        assert bool((got[geo.gy:] == 0).all()), "a replica no workgroup maps to has been written"
        S, b = O.reduce(p.g, p.y, p.vecs, self.act, geo)
        for k, nm in enumerate(("-s1", "-s2")):
            _report(what + nm, p.dt, *O.check(got.sum(0)[k], S[k], b[k]), case)
        return got.clone()

    def verify_apply(self, what, case):
        p = self.p
        self.inputs_untouched()
        self.red.assert_untouched()
        self.o.assert_outside_untouched()
        S, e_fold = O.totals(self.red_h)
        tgt, b = O.apply(p.g, p.y, p.vecs, self.act, S, p.P, BC.DTYPES[p.dt], p.old if self.accum else None)
        _report(what, p.dt, *O.check(BC.get_rows(self.o), tgt, b), case)
        if self.dg is not None:                      # grid row 0 only: the bound of ONE addition
            for f, k, old in ((self.dg, 1, 0.25), (self.db, 0, -0.5)):
                f.assert_outside_untouched()
                _report(what + ("-dgamma" if k else "-dbeta"), "f32", *O.check(f.t.cpu(), *O.param_bound(S[k], e_fold[k], torch.full((p.C,), old))), case)
        return _bits(self.o)


@pytest.mark.parametrize("sid,dt", BC.TRAIN)
def test_reduce(sid, dt):
    BC.assert_geometry(sid, dt)
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        slots = BC.REDUCE_SLOTS[i % 3]
        lays = _lays(i)
        r = Bwd(p, act, lays, slots=slots, aux=False, out=False)
        r.reduce()
        r.verify_reduce("reduce-" + act, "%s %s slots %d" % (sid, "/".join(lays[:2]), slots))


def test_reduce_capped_grid():
    BC.assert_geometry(BC.BIG.id, "bf16")
    r = Bwd(BC.problem(BC.BIG.id, "bf16"), "leaky", ("slice", "tight", "tight"), slots=16, aux=False, out=False)
    r.reduce()
    r.verify_reduce("reduce-leaky", BC.BIG.id)


@pytest.mark.parametrize("C", [8, 24, 264])
def test_params(C):
    """dyk_bn_bwd_params: replica 0 holds the totals afterwards, the other replicas are as they were; dgamma / dbeta null or set"""
    for slots in BC.REDUCE_SLOTS + [33, 256]:
        for both in (True, False):
            red_h = BC.replicas(C, slots, 577)
            red = Flat(red_h).arm()
            dg, db = Flat(torch.full((C,), 0.25)).arm(), Flat(torch.full((C,), -0.5)).arm()
            _sync_ok(_lib().dyk_bn_bwd_params(red.t.data_ptr(), dg.t.data_ptr() if both else None, db.t.data_ptr(), C, slots, None), "dyk_bn_bwd_params")
            red.assert_outside_untouched()
            got = red.t.cpu()
            assert torch.equal(got[1:], red_h[1:]), "a replica other than the first has been written"
            S, e_fold = O.totals(red_h)
            case = "C%d slots %d" % (C, slots)
            _report("params-totals", "f64", *O.check(got[0], S, e_fold), case)
            db.assert_outside_untouched()
            _report("params-dbeta", "f32", *O.check(db.t.cpu(), *O.param_bound(S[0], e_fold[0], torch.full((C,), -0.5))), case)
            if both:
                dg.assert_outside_untouched()
                _report("params-dgamma", "f32", *O.check(dg.t.cpu(), *O.param_bound(S[1], e_fold[1], torch.full((C,), 0.25))), case)
            else:
                dg.assert_untouched()


@pytest.mark.parametrize("sid,dt", BC.TRAIN)
def test_apply(sid, dt):
    """the seven activations (linear: a stored da) over every replica count, ACCUM or not, aux / aux2 set or null, the eight layout
    combinations; the in-place form; 16 replicas as columns of a wider reduction (H, W)"""
    BC.assert_geometry(sid, dt)
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        slots = BC.APPLY_SLOTS[i % len(BC.APPLY_SLOTS)]
        lays, accum, aux = _lays(i), bool(i & 1), i % 3 != 2
        a = Bwd(p, act, lays, BC.replicas(p.C, slots, p.P), slots, accum=accum, aux=aux)
        a.apply()
        want = a.verify_apply("apply-" + act, "%s %s slots %d accum%d aux%d" % (sid, "/".join(lays), slots, accum, aux))
        if i % 3 == 0 and not accum:
            q = Bwd(p, act, lays, BC.replicas(p.C, slots, p.P), slots, aux=aux, inplace=True)
            q.apply()
            assert torch.equal(q.verify_apply("apply-inplace-" + act, sid), want), "the in-place form differs from the out-of-place one"
    for accum in (False, True):
        a = Bwd(p, "leaky", _lays(3), BC.replicas(p.C, 16, p.P), 16, route=True, accum=accum)
        a.apply()
        a.verify_apply("apply-route", "%s accum%d" % (sid, accum))


def test_apply_capped_grid():
    BC.assert_geometry(BC.BIG.id, "bf16")
    p = BC.problem(BC.BIG.id, "bf16")
    a = Bwd(p, "leaky", ("tight", "slice", "tight"), BC.replicas(p.C, 16, p.P), 16, accum=True)
    a.apply()
    a.verify_apply("apply-leaky", BC.BIG.id)


@pytest.mark.parametrize("act", [a for a in BC.ACTS if a != "mish"])
def test_kink_field(act):
    """scale 1, shift 0, gradient 1, one pixel, one value per channel: 0, -0, the smallest normals, +-3, 6 and their bf16 neighbours.  t is
    exact, so the derivative is the convention's, bit for bit: in the first sum of the reduce and in the dy the apply stores (totals 0)"""
    y, g, vecs = BC.kink_field()
    p = BC.Problem("kink", "bf16", 1, 16, y, g, y, y, vecs)
    want = BC.kink_da(act)
    exact = ((y.abs() >= 3) | torch.tensor(act != "hard-swish")).view(-1)       # (hard-swish between the knees: y / 3 + 0.5, fused or not)
    r = Bwd(p, act, aux=False, out=False)
    r.reduce()
    red = r.verify_reduce("kink-reduce-" + act, "kink")
    assert torch.equal(red[0, 0].float()[exact], want[0][exact]), "%s: derivative at a kink %s, convention %s" % (act, red[0, 0], want[0])
    a = Bwd(p, act, aux=False)
    a.apply()
    dy = a.verify_apply("kink-apply-" + act, "kink").view(-1)
    assert O.same_bits(dy[exact], want[0].bfloat16()[exact]) == 0, "%s: dy at a kink %s, convention %s" % (act, dy, want[0])


# ---------------------------------------------------------------------------------------------------- two-problem launches
def test_twin_launches():
    """DykEwDesc.twin / DykBnFinalizeDesc.twin, gridDim.z = 2: two different problems give the bits of two single launches, for all five kernels"""
    p = BC.problem("577", "bf16")
    q = _alt(p)
    lays = ("slice", "tight", "slice")
    # forward
    singles = []
    for pr, alt in ((p, False), (p, True)):
        f = Fwd(pr, "mish", lays, True, alt=alt)
        f.launch()
        singles.append(f.verify("twin-single-fwd", "577"))
    x, y = Fwd(p, "mish", lays, True), Fwd(p, "mish", lays, True, alt=True)
    _pair(Fwd.launch, x, y)
    assert torch.equal(x.verify("twin-fwd", "577"), singles[0]) and torch.equal(y.verify("twin-fwd", "577 second"), singles[1])
    # finalize
    fp, fq = BC.fin_problem(264, 577, 33), BC.fin_problem(264, 577, 33, seed=1)
    singles = []
    for pr in (fp, fq):
        f = Fin(pr)
        f.launch()
        singles.append(f.verify("twin-single-finalize", "577", rearmed=True))
    x, y = Fin(fp), Fin(fq)
    _pair(Fin.launch, x, y)
    for f, want in ((x, singles[0]), (y, singles[1])):
        assert all(torch.equal(a, b) for a, b in zip(f.verify("twin-finalize", "577", rearmed=True), want))
    # fused forward
    fp, fq = BC.fin_problem(264, 577, 7), BC.fin_problem(264, 577, 7, seed=1)
    singles = []
    for pr, fi, alt in ((p, fp, False), (p, fq, True)):
        f = Fwd(pr, "leaky", lays, True, alt=alt, fin=Fin(fi))
        f.launch()
        singles.append((f.verify("twin-single-fused", "577"), f.fin.verify("twin-single-fused", "577", rearmed=False)))
    x, y = Fwd(p, "leaky", lays, True, fin=Fin(fp)), Fwd(p, "leaky", lays, True, alt=True, fin=Fin(fq))
    x.fin.d.twin = ctypes.addressof(y.fin.d)
    _pair(Fwd.launch, x, y)
    for f, (want, fw) in ((x, singles[0]), (y, singles[1])):
        assert torch.equal(f.verify("twin-fused", "577"), want)
        assert all(torch.equal(a, b) for a, b in zip(f.fin.verify("twin-fused", "577", rearmed=False), fw))
    # reduce (one workgroup per replica and channel group at 577 pixels: gy = 10 <= 16, so the fp64 atomics have one order) and apply
    singles = []
    for pr in (p, q):
        r = Bwd(pr, "hard-swish", lays, slots=16, aux=False, out=False)
        r.reduce()
        singles.append(r.verify_reduce("twin-single-reduce", "577"))
    x, y = (Bwd(pr, "hard-swish", lays, slots=16, aux=False, out=False) for pr in (p, q))
    _pair(Bwd.reduce, x, y)
    assert torch.equal(x.verify_reduce("twin-reduce", "577"), singles[0]) and torch.equal(y.verify_reduce("twin-reduce", "577 second"), singles[1])
    reds = (BC.replicas(264, 25, 577), BC.replicas(264, 25, 577, seed=1))
    singles = []
    for pr, rd in zip((p, q), reds):
        a = Bwd(pr, "relu6", lays, rd, 25, accum=True)
        a.apply()
        singles.append((a.verify_apply("twin-single-apply", "577"), a.dg.t.cpu().clone(), a.db.t.cpu().clone()))
    x, y = (Bwd(pr, "relu6", lays, rd, 25, accum=True) for pr, rd in zip((p, q), reds))
    _pair(Bwd.apply, x, y)
    for a, want in ((x, singles[0]), (y, singles[1])):
        assert torch.equal(a.verify_apply("twin-apply", "577"), want[0]) and torch.equal(a.dg.t.cpu(), want[1]) and torch.equal(a.db.t.cpu(), want[2])


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """no launch: C % EPV, ld % EPV, null operands, f->C != d->C, f16 on the training kernels, a twin that differs in a non-pointer field, a
    twin paired on one descriptor only; DYK_EW_SKIP returns OK and writes nothing"""
    lib, L = _lib(), _L()
    p = BC.problem("35", "bf16")
    calls = {"fwd": lambda o: lib.dyk_bn_act_fwd(ctypes.byref(o.d), None), "reduce": lambda o: lib.dyk_bn_act_bwd_reduce(ctypes.byref(o.d), None),
             "apply": lambda o: lib.dyk_bn_act_bwd_apply(ctypes.byref(o.d), None),
             "fused": lambda o: lib.dyk_bn_finalize_act_fwd(ctypes.byref(o.fin.d), ctypes.byref(o.d), None)}

    def make(kind):
        if kind == "fwd":
            return Fwd(p, "leaky")
        if kind == "fused":
            return Fwd(p, "leaky", fin=Fin(BC.fin_problem(p.C, p.P, 4)))
        return Bwd(p, "leaky", red=BC.replicas(p.C, 4, p.P), slots=4)

    def refused(kind, want, **fields):
        o = make(kind)
        for k, v in fields.items():
            setattr(o.d, k, v)
        assert calls[kind](o) == want, "%s with %s" % (kind, fields)
        torch.cuda.synchronize()
        for f in (o.o, getattr(o, "red", None), getattr(o, "dg", None), getattr(o, "db", None)):
            if f is not None:
                f.assert_untouched()
        if kind == "fused":
            for f in (o.fin.stats, o.fin.scale, o.fin.shift, o.fin.rm, o.fin.rv):
                f.assert_untouched()

    for kind in calls:
        refused(kind, ERR_ARG, C=p.C - 4)                                  # C % EPV
        refused(kind, ERR_ARG, lda=p.C + 4)                                # ld % EPV
        refused(kind, ERR_ARG, a=None)
        refused(kind, ERR_ARG, npix=0)
        if kind != "fwd":
            refused(kind, ERR_UNSUPPORTED, dtype=L.DYK_F16)
        if kind != "reduce":
            refused(kind, ERR_ARG, ldo=p.C + 4)
            refused(kind, ERR_ARG, out=None)
    refused("fwd", ERR_ARG, ldb=p.C + 4)
    for kind in ("reduce", "apply"):
        for k in ("b", "red", "p0", "p1", "p2", "p3"):
            refused(kind, ERR_ARG, **{k: None})
        refused(kind, ERR_ARG, ldb=p.C + 4)
    refused("fused", ERR_ARG, C=p.C + 8)                                   # f->C != d->C
    for k in ("stats", "scale", "shift"):
        o = make("fused")
        setattr(o.fin.d, k, None)
        assert calls["fused"](o) == ERR_ARG and lib.dyk_bn_finalize(ctypes.byref(o.fin.d), None) == ERR_ARG
    o = make("fused")
    o.fin.d.count = 0
    assert calls["fused"](o) == ERR_ARG and lib.dyk_bn_finalize(ctypes.byref(o.fin.d), None) == ERR_ARG
    # a twin that differs in a non-pointer field; a twin with another set of optional operands; a twin on one descriptor only
    for kind in ("fwd", "reduce", "apply"):
        x, y = make(kind), make(kind)
        y.d.act = L.ACT_CODES["relu"]
        assert _pair(calls[kind], x, y) == ERR_ARG
        y = make(kind)
        y.d.p1 = None
        assert _pair(calls[kind], x, y) == ERR_ARG
    x, y = Fin(BC.fin_problem(24, 35, 4)), Fin(BC.fin_problem(24, 35, 4, seed=1))
    y.d.eps = 1e-3
    assert _pair(lambda f: lib.dyk_bn_finalize(ctypes.byref(f.d), None), x, y) == ERR_ARG
    x, y = make("fused"), make("fused")
    assert _pair(calls["fused"], x, y) == ERR_ARG                          # the elementwise descriptors paired, the finalize ones not
    x.fin.d.twin = ctypes.addressof(y.fin.d)
    assert calls["fused"](x) == ERR_ARG                                    # and the other way round
    torch.cuda.synchronize()
    for o in (x, y):
        o.o.assert_untouched()
        o.fin.stats.assert_untouched()
    # DYK_EW_SKIP: done inside the consumer; OK, nothing written
    a = make("apply")
    a.d.flags = L.EW_SKIP
    _sync_ok(calls["apply"](a), "dyk_bn_act_bwd_apply(SKIP)")
    for f in (a.o, a.red, a.dg, a.db):
        f.assert_untouched()
