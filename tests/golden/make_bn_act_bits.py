"""Generates tests/golden/bn_act_bits.json: sha256 digests of what the BatchNorm/activation kernels of csrc/bn_act.hip and the
squeeze-excitation and max-pool kernels of csrc/elementwise.hip leave in memory, taken from the library named by DYK_LIB (default: the
in-tree build) on an MI355X.  tests/test_gpu_bn_act_bits.py holds the library under test to every digest.  The committed file was
written by the commit BEFORE these kernels moved onto the shared pieces of csrc/ew_strip.h; regenerate it only when the bits of a
kernel are meant to change.

The problems are those of tests/bn_act_cases.py and tests/elementwise_cases.py, the buffers those of the two element suites
(sentinel-filled; guard rows, padding channels and frames inside every digest).  One case is a group of launches; per launch one
digest over every buffer the launch may touch, inputs included:
  fin      dyk_bn_finalize, FIN_CASES x FIN_SLOTS               fold     dyk_bn_fold, C = 1, 24, 264 with and without gamma / beta
  params   dyk_bn_bwd_params, the cases of test_params
  fwd      dyk_bn_act_fwd, SMALL x seven activations x residual or not x all-tight | all-slice rows
  fused    dyk_bn_finalize_act_fwd, TRAIN x seven activations x FUSED_SLOTS
  apply    dyk_bn_act_bwd_apply, TRAIN x seven activations x APPLY_SLOTS, plain and DYK_EW_ACCUM, aux / aux2 set; one launch on the
           columns of a wider reduction
  reduce   dyk_bn_act_bwd_reduce, TRAIN x seven activations with slots = the launch's own gy: every replica address receives exactly
           ONE atomic onto zero, so the bits are fixed.  (gy > slots has no fixed summation order: it stays under the fp64 bounds of
           test_reduce.)
  big      65537 pixels, bf16, leaky: forward, fused forward, apply     twin     one two-problem launch of each kernel that takes one
  se_pool  SE_POOL_C x SE_POOL_MAPS, with and without b, with and without the split scratch
  se_scale SE_SCALE_C x SE_SCALE_MAPS: plain, with p1, DYK_EW_ACCUM, and with the BatchNorm-backward reduce at slots = the launch's
           workgroup count gy * nz (one atomic per address again); SE_SCALE_LOOP: several images per workgroup
  pool     max pool forward with arg-max and backward: tile_matrix(), GENERIC_KS, STRIDED
Every entry also carries a digest of its inputs: a test that fails there says that the inputs changed, not the kernel.

    DYK_LIB=/path/to/libdyk_hip.so python tests/golden/make_bn_act_bits.py [--out FILE]
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "double-yolo-kaist_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "bn_act_bits.json")
FOLD_C = [1, 24, 264]
PARAMS_C = [8, 24, 264]
FWD_LAYS = [("tight",) * 3, ("slice",) * 3]


def _t(t):
    import torch
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()


def _E():
    import test_gpu_bn_act_elements as E
    return E


def _W():
    import test_gpu_elementwise_elements as W
    return W


class Rec:
    """collects one case: every buffer's armed contents go into the input digest, its contents after the launch into the launch's"""

    def __init__(self, *what):
        self.h = hashlib.sha256(repr(what).encode())
        self.out = {}

    def add(self, name, bufs, launch, note=""):
        bufs = [b for i, b in enumerate(bufs) if b is not None and all(b is not o for o in bufs[:i])]
        self.h.update(("%s|%s|%d" % (name, note, len(bufs))).encode())
        for b in bufs:
            self.h.update(_t(b.before))
        launch()
        assert name not in self.out, name
        h = hashlib.sha256()
        for b in bufs:
            h.update(_t(b.flat))
        self.out[name] = h.hexdigest()

    def done(self):
        return self.h.hexdigest(), self.out


def _fin_bufs(f):
    return [f.stats, f.gamma, f.beta, f.rm, f.rv, f.scale, f.shift, f.mean, f.rstd]


def _fwd_bufs(f):
    return [f.a, f.b, f.o, f.fsc, f.fsh] + (_fin_bufs(f.fin) if f.fin is not None else [])


def _bwd_bufs(b):
    return [b.a, b.b, b.o, b.vecs, b.red, b.dg, b.db]


# ---------------------------------------------------------------------------------------------- csrc/bn_act.hip
def run_fin(C, count):
    import bn_act_cases as BC
    E, r = _E(), Rec("fin", C, count)
    for slots in BC.FIN_SLOTS:
        f = E.Fin(BC.fin_problem(C, count, slots))
        r.add("slots%d" % slots, _fin_bufs(f), f.launch)
    f = E.Fin(BC.fin_problem(C, count, 4), False, False, False, False)
    r.add("null", _fin_bufs(f), f.launch)
    return r.done()


def run_fold():
    import bn_act_cases as BC
    E, r = _E(), Rec("fold")
    for C in FOLD_C:
        g, b, rm, rv = BC.fold_problem(C)
        for gg, bb in ((g, b), (None, b), (g, None), (None, None)):
            ins = [E.Flat(v).arm() if v is not None else None for v in (gg, bb, rm, rv)]
            sc, sh = E._out_vec(C), E._out_vec(C)
            ptr = [f.t.data_ptr() if f is not None else None for f in ins]
            r.add("C%d-gamma%d-beta%d" % (C, gg is not None, bb is not None), ins + [sc, sh], lambda: E._sync_ok(
                E._lib().dyk_bn_fold(ptr[0], ptr[1], ptr[2], ptr[3], BC.EPS, sc.t.data_ptr(), sh.t.data_ptr(), C, None), "dyk_bn_fold"))
    return r.done()


def run_params(C):
    import torch
    import bn_act_cases as BC
    E, r = _E(), Rec("params", C)
    for slots in BC.REDUCE_SLOTS + [33, 256]:
        for both in (True, False):
            red = E.Flat(BC.replicas(C, slots, 577)).arm()
            dg, db = E.Flat(torch.full((C,), 0.25)).arm(), E.Flat(torch.full((C,), -0.5)).arm()
            r.add("slots%d-dgamma%d" % (slots, both), [red, dg, db], lambda: E._sync_ok(E._lib().dyk_bn_bwd_params(
                red.t.data_ptr(), dg.t.data_ptr() if both else None, db.t.data_ptr(), C, slots, None), "dyk_bn_bwd_params"))
    return r.done()


def run_fwd(sid, dt):
    import bn_act_cases as BC
    E, r = _E(), Rec("fwd", sid, dt)
    p = BC.problem(sid, dt)
    for act in BC.ACTS:
        for res in (True, False):
            for lays in FWD_LAYS:
                f = E.Fwd(p, act, lays, res)
                r.add("%s-res%d-%s" % (act, res, lays[0]), _fwd_bufs(f), f.launch)
    return r.done()


def _fused(p, act, slots, lays, res, alt=False, seed=0):
    import bn_act_cases as BC
    E = _E()
    return E.Fwd(p, act, lays, res, alt=alt, fin=E.Fin(BC.fin_problem(p.C, p.P, slots, seed)))


def run_fused(sid, dt):
    import bn_act_cases as BC
    E, r = _E(), Rec("fused", sid, dt)
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        for k, slots in enumerate(BC.FUSED_SLOTS):
            f = _fused(p, act, slots, E._lays(i + k), bool((i + k) & 1))
            r.add("%s-slots%d" % (act, slots), _fwd_bufs(f), f.launch)
    return r.done()


def run_apply(sid, dt):
    import bn_act_cases as BC
    E, r = _E(), Rec("apply", sid, dt)
    p = BC.problem(sid, dt)
    for i, act in enumerate(BC.ACTS):
        for k, slots in enumerate(BC.APPLY_SLOTS):
            for accum in (False, True):
                a = E.Bwd(p, act, E._lays(i + k), BC.replicas(p.C, slots, p.P), slots, accum=accum)
                r.add("%s-slots%d-accum%d" % (act, slots, accum), _bwd_bufs(a), a.apply)
    a = E.Bwd(p, "leaky", E._lays(3), BC.replicas(p.C, 16, p.P), 16, route=True)
    r.add("route", _bwd_bufs(a), a.apply)
    return r.done()


def run_reduce(sid, dt):
    """slots = gy: workgroup row y alone adds to replica y, once per address, onto zero"""
    import bn_act_cases as BC
    from oracle import bn_act as O
    E, r = _E(), Rec("reduce", sid, dt)
    p = BC.problem(sid, dt)
    gy = O.reduce_grid(p.C, p.P, dt).gy
    for i, act in enumerate(BC.ACTS):
        b = E.Bwd(p, act, E._lays(i), slots=gy, aux=False, out=False)
        r.add(act, _bwd_bufs(b), b.reduce, "slots%d" % gy)
    return r.done()


def run_big(kind):
    import bn_act_cases as BC
    E, r = _E(), Rec("big", kind)
    p = BC.problem(BC.BIG.id, "bf16")
    if kind == "fwd":
        f = E.Fwd(p, "leaky", ("tight", "slice", "slice"), True)
        r.add(kind, _fwd_bufs(f), f.launch)
    elif kind == "fused":
        f = _fused(p, "leaky", 32, ("slice", "tight", "tight"), True)
        r.add(kind, _fwd_bufs(f), f.launch)
    else:
        a = E.Bwd(p, "leaky", ("tight", "slice", "tight"), BC.replicas(p.C, 16, p.P), 16, accum=True)
        r.add(kind, _bwd_bufs(a), a.apply)
    return r.done()


def run_twin():
    """the launches of test_twin_launches: both problems' buffers in one digest (reduce: gy = 10 <= 16 replicas)"""
    import bn_act_cases as BC
    E, r = _E(), Rec("twin")
    p = BC.problem("577", "bf16")
    q = E._alt(p)
    lays = ("slice", "tight", "slice")
    x, y = E.Fwd(p, "mish", lays, True), E.Fwd(p, "mish", lays, True, alt=True)
    r.add("fwd", _fwd_bufs(x) + _fwd_bufs(y), lambda: E._pair(E.Fwd.launch, x, y))
    fx, fy = E.Fin(BC.fin_problem(264, 577, 33)), E.Fin(BC.fin_problem(264, 577, 33, seed=1))
    r.add("finalize", _fin_bufs(fx) + _fin_bufs(fy), lambda: E._pair(E.Fin.launch, fx, fy))
    ux, uy = _fused(p, "leaky", 7, lays, True), _fused(p, "leaky", 7, lays, True, alt=True, seed=1)
    ux.fin.d.twin = ctypes.addressof(uy.fin.d)
    r.add("fused", _fwd_bufs(ux) + _fwd_bufs(uy), lambda: E._pair(E.Fwd.launch, ux, uy))
    rx, ry = (E.Bwd(pr, "hard-swish", lays, slots=16, aux=False, out=False) for pr in (p, q))
    r.add("reduce", _bwd_bufs(rx) + _bwd_bufs(ry), lambda: E._pair(E.Bwd.reduce, rx, ry))
    ax, ay = (E.Bwd(pr, "relu6", lays, BC.replicas(264, 25, 577, seed=s), 25, accum=True) for s, pr in enumerate((p, q)))
    r.add("apply", _bwd_bufs(ax) + _bwd_bufs(ay), lambda: E._pair(E.Bwd.apply, ax, ay))
    return r.done()


# ---------------------------------------------------------------------------------------------- csrc/elementwise.hip
def run_se_pool(dt, C):
    import torch
    import elementwise_cases as EC
    W, r = _W(), Rec("se_pool", dt, C)
    L, B = W._L(), 2
    for H, Wd in EC.SE_POOL_MAPS:
        x, y = EC.rand_tensor(B, C, H, Wd, dt, 41), EC.rand_tensor(B, C, H, Wd, dt, 42)
        for i, (second, scratch) in enumerate(((False, False), (False, True), (True, True), (True, False))):
            lay = ("tight", "slice")[i % 2]
            xb = EC.nhwc(x, dt, lay)
            yb = EC.nhwc(y, dt, W._other(lay)) if second else None
            pooled = W.Flat(torch.zeros(B, C), fill=W.NAN).arm()
            sc = W.Flat(torch.zeros(L.SE_POOL_SPLITS * B * C), fill=W.NAN).arm()
            d = W._desc(dt, C, a=xb, b=yb, B=B, H=H, W=Wd, alpha=0.5 if second else 1.0 / (H * Wd), aux2=sc if scratch else None)
            r.add("%dx%d-b%d-scratch%d" % (H, Wd, second, scratch), [xb, yb, pooled, sc],
                  lambda: W._ok(W._lib().dyk_se_pool(ctypes.byref(d), W._ptr(pooled), None), "dyk_se_pool"))
    return r.done()


def _se_scale(r, name, dt, B, C, H, Wd, has_p1, accumulate, lay, act=None):
    """act: with the BatchNorm-backward reduce, slots = gy * nz workgroups: one atomic per replica address"""
    import torch
    import elementwise_cases as EC
    W = _W()
    L = W._L()
    dz, yraw, old, p0v, p1v, vecs = EC.se_reduce_problem(B, C, H, Wd, dt)
    abuf, obuf = EC.nhwc(dz, dt, lay), EC.nhwc(old, dt, W._other(lay), fill=accumulate)
    p0, p1 = W.Flat(p0v).arm(), W.Flat(p1v).arm() if has_p1 else None
    ybuf = p2 = red = None
    slots = 0
    if act is not None:
        _, _, _, gy, nz = EC.se_scale_geo(C, dt, B, H * Wd, True)
        slots = gy * nz
        ybuf, p2 = EC.nhwc(yraw, dt, W._other(lay)), W.Flat(vecs).arm()
        red = W.Flat(torch.zeros(slots, 2, C, dtype=torch.float64)).arm()
    d = W._desc(dt, C, a=abuf, b=ybuf, out=obuf, B=B, H=H, W=Wd, alpha=1.0 / (H * Wd), p0=p0, p1=p1, p2=p2, red=red,
                act=L.ACT_CODES[act or "linear"], slots=slots, flags=L.EW_ACCUM if accumulate else 0)
    r.add(name, [abuf, ybuf, obuf, p0, p1, p2, red], lambda: W._ok(W._lib().dyk_se_scale(ctypes.byref(d), None), "dyk_se_scale"),
          "slots%d" % slots)


def run_se_scale(dt, C):
    import elementwise_cases as EC
    from oracle import elementwise as O
    r = Rec("se_scale", dt, C)
    for H, Wd in EC.SE_SCALE_MAPS:
        for i, (has_p1, accumulate) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            _se_scale(r, "%dx%d-p1%d-accum%d" % (H, Wd, has_p1, accumulate), dt, 2, C, H, Wd, has_p1, accumulate, ("tight", "slice")[i % 2])
        for i, act in enumerate(O.REDUCE_ACTS):
            _se_scale(r, "%dx%d-reduce-%s" % (H, Wd, act), dt, 2, C, H, Wd, i % 2 == 0, i % 4 >= 2, ("tight", "slice")[i % 2], act)
    return r.done()


def run_se_scale_loop():
    import elementwise_cases as EC
    r = Rec("se_scale_loop")
    B, C, H, Wd = EC.SE_SCALE_LOOP
    assert EC.se_scale_geo(C, "bf16", B, H * Wd, True)[4] < B
    _se_scale(r, "hard-swish", "bf16", B, C, H, Wd, True, False, "tight", "hard-swish")
    return r.done()


def _pool(r, name, dt, B, C, H, Wd, k, stride, lay):
    """forward with arg-max, then (bf16 | f32) the backward, store and accumulate, on the codes the forward left"""
    import torch
    import elementwise_cases as EC
    W = _W()
    x = EC.pool_input(B, C, H, Wd)
    Ho, Wo = EC.pool_shape(H, Wd, k, stride)
    if Ho == 0 or Wo == 0:
        return
    xin = EC.nhwc(x, dt, lay)
    out = EC.nhwc(torch.zeros(B, C, Ho, Wo), dt, W._other(lay), fill=False)
    am = W.Flat(torch.zeros(B, Ho, Wo, C, dtype=torch.uint8), fill=255).arm()
    d = W._desc(dt, C, a=xin, out=out, B=B, H=H, W=Wd, k=k, slots=stride)
    r.add(name + "-fwd", [xin, out, am], lambda: W._ok(W._lib().dyk_maxpool_fwd(ctypes.byref(d), W._ptr(am), None), "dyk_maxpool_fwd"))
    if dt == "f16":
        return
    for accumulate in (False, True):
        g = EC.nhwc(EC.pool_grad(B, C, Ho, Wo, dt, accumulate), dt, lay)
        dx = EC.nhwc(EC.rand_tensor(B, C, H, Wd, dt, 9), dt, W._other(lay), fill=accumulate)
        am.arm()
        db = W._desc(dt, C, a=g, out=dx, B=B, H=H, W=Wd, k=k, slots=stride, flags=W._L().EW_ACCUM if accumulate else 0)
        r.add("%s-bwd-accum%d" % (name, accumulate), [g, am, dx],
              lambda: W._ok(W._lib().dyk_maxpool_bwd(ctypes.byref(db), W._ptr(am), None), "dyk_maxpool_bwd"))


def run_pool_tile(H, Wd):
    import elementwise_cases as EC
    r = Rec("pool-tile", H, Wd)
    for k in EC.TILE_KS:
        for dt, C, B, lay in EC.tile_variants(H, Wd, k):
            _pool(r, "k%d-%s-c%d" % (k, dt, C), dt, B, C, H, Wd, k, 1, lay)
    return r.done()


def run_pool_generic():
    import elementwise_cases as EC
    r = Rec("pool-generic")
    H, Wd = EC.GENERIC_MAP
    for k in EC.GENERIC_KS:
        for dt, C, lay in (("bf16", 8, "tight"), ("f32", 4, "slice"), ("f16", 8, "slice"), ("bf16", 24, "slice")):
            _pool(r, "k%d-%s-c%d" % (k, dt, C), dt, 1, C, H, Wd, k, 1, lay)
    return r.done()


def run_pool_strided(H, Wd):
    import elementwise_cases as EC
    r = Rec("pool-strided", H, Wd)
    for k, stride in EC.STRIDED:
        for dt, C, lay in (("bf16", 8, "slice"), ("f32", 4, "tight"), ("f16", 16, "tight")):
            _pool(r, "k%d-s%d-%s-c%d" % (k, stride, dt, C), dt, 2, C, H, Wd, k, stride, lay)
    return r.done()


# ---------------------------------------------------------------------------------------------- the table of cases
def cases():
    """-> {id: (runner, arguments)}"""
    import bn_act_cases as BC
    import elementwise_cases as EC
    E = _E()
    out = {}
    for C, n in E.FIN_CASES:
        out["fin-C%d-n%d" % (C, n)] = (run_fin, (C, n))
    out["fold"] = (run_fold, ())
    for C in PARAMS_C:
        out["params-C%d" % C] = (run_params, (C,))
    for sid, dt in BC.SMALL:
        out["fwd-%s-%s" % (sid, dt)] = (run_fwd, (sid, dt))
    for name, fn in (("fused", run_fused), ("apply", run_apply), ("reduce", run_reduce)):
        for sid, dt in BC.TRAIN:
            out["%s-%s-%s" % (name, sid, dt)] = (fn, (sid, dt))
    for kind in ("fwd", "fused", "apply"):
        out["big-" + kind] = (run_big, (kind,))
    out["twin"] = (run_twin, ())
    for dt, C in EC.SE_POOL_C:
        out["se_pool-%s-c%d" % (dt, C)] = (run_se_pool, (dt, C))
    for dt, C in EC.SE_SCALE_C:
        out["se_scale-%s-c%d" % (dt, C)] = (run_se_scale, (dt, C))
    out["se_scale-loop"] = (run_se_scale_loop, ())
    for H, Wd in EC.TILE_MAPS:
        out["pool-tile-%dx%d" % (H, Wd)] = (run_pool_tile, (H, Wd))
    out["pool-generic"] = (run_pool_generic, ())
    for H, Wd in EC.STRIDED_MAPS:
        out["pool-strided-%dx%d" % (H, Wd)] = (run_pool_strided, (H, Wd))
    return out


def run_case(fn, args):
    """-> (digest of the inputs, {launch: digest})"""
    return fn(*args)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library, so that both use the HIP runtime torch brings)
    from dyk import lib as L
    lib = L.load()
    table = {}
    for cid, (fn, args) in cases().items():
        table[cid] = dict(zip(("in", "out"), run_case(fn, args)))
    with open(a.out, "w") as f:
        f.write('{"library": "%s",\n "cases": {\n' % lib.dyk_build_sha().decode())
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()))
        f.write("\n }}\n")
    print("%s: %d cases, %d launches, library %s" % (a.out, len(table), sum(len(v["out"]) for v in table.values()), lib.dyk_build_sha().decode()))


if __name__ == "__main__":
    main()
