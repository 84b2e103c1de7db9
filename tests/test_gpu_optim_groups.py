"""dyk_adam_step_groups / dyk_sgd_step_groups (csrc/optim.hip) at their own ABI: DykOptimDesc + DykOptimGroups built by hand over
plain CUDA tensors, no model.  Every element of p, m, v is held to the grouped fp64 reference of tests/optim_groups_ref.py within
its derived bound (tests/test_optim_groups_reference.py shows what that bound lets through and what it catches); equality with
dyk_adam_step / dyk_sgd_step and their guarded forms, sub-range launches, the bf16 copy, skipped steps and the argument checks
are compared bit for bit.  Buffers, guard bands and the per-element comparison are those of tests/test_gpu_optim.py."""
import ctypes

import numpy as np
import pytest
import torch

import optim_groups_ref as R
from oracle.optim import input_family
from test_gpu_optim import BIG, ERR_ARG, Bufs, _bf16_specials, _h, _i32, _within

pytestmark = pytest.mark.gpu

f32 = np.float32
ERR_UNSUPPORTED = -3                           # DYK_ERR_UNSUPPORTED (include/dyk_hip.h)
SWEEP = 8192 * 256 * 4                         # elements of the first grid-stride sweep; BIG - SWEEP = 1028
L2 = [dict(lr=1e-3, weight_decay=5e-4), dict(lr=1e-3, weight_decay=0.0), dict(lr=2e-3, weight_decay=0.0)]
ADAMW = dict(lr=1e-3, weight_decay=1e-2, decoupled=True)
SHARED = {"adam": dict(beta1=0.937, beta2=0.999, eps=1e-8), "sgd": dict(beta1=0.937)}
IGNORED = dict(lr=7.0, weight_decay=3.0)       # what the descriptor carries in these two fields must not matter
_CACHE = {}


def groups_of(kind):
    return L2 + [ADAMW] if kind == "adam" else L2


def block_map(ngroups):
    """BIG elements in a few long runs, with group changes inside the first sweep (at entries that are no multiple of the
    block's 1024 elements), across the sweep boundary, and inside the ragged second sweep; frozen runs in between"""
    gm = np.zeros(BIG, np.uint8)
    e = 64
    edges = [0, 1000 * e + e, 1003 * e, 50000 * e + 7 * e, SWEEP - 9 * e, SWEEP + 512, SWEEP + 768, SWEEP + 1024, BIG]
    values = [1, 0, 2, 3, ngroups, 1, 0, 2]                 # the last run is the 4-element entry behind the last full one
    for lo, hi, k in zip(edges, edges[1:], values):
        gm[lo:hi] = k
    assert len(set(values)) == ngroups + 1
    return gm


def layout(name, kind):
    """-> (n, group map, groups)"""
    groups = groups_of(kind)
    if name == "one":
        return 4, np.ones(4, np.uint8), groups[:1]
    if name == "interleaved":
        return 64 * 50, R.interleaved_map(64 * 50, len(groups)), groups
    return BIG, block_map(len(groups)), groups


def inputs(kind, n, seed, beta1, grad_scale):
    """input_family, computed once per process and shared (do not modify)"""
    key = (kind, n, seed, grad_scale)
    if key not in _CACHE:
        p, g, m, v = input_family(n, seed, kind, beta1, grad_scale)
        if kind == "sgd":                                   # the kernel must neither read nor write v
            v = np.full(n, np.nan, np.float32)
            _i32(v)[:] = 0x7fc12345
        _CACHE[key] = dict(p=p, g=g, m=m, v=v)
    return _CACHE[key]


def table_of(groups):
    from dyk import lib as L
    t = L.DykOptimGroups()
    t.count = len(groups)
    for k, (lr, wd, dm, flags) in enumerate(R.table(groups)):
        t.g[k].lr, t.g[k].weight_decay, t.g[k].decay_mul, t.g[k].flags = lr, wd, dm, flags
    return t


def record(h, applied, coef=1.0, skip=0):
    """a DykGradGuardRec as dyk_grad_stats leaves it (include/dyk_hip.h), in device memory"""
    from dyk import lib as L
    r = L.DykGradGuardRec()
    r.coef, r.skip, r.applied = coef, skip, applied
    r.bc1 = f32(1.0 - float(f32(h["beta1"])) ** applied)
    r.bc2_sqrt = f32(np.sqrt(1.0 - float(f32(h.get("beta2", 0.0))) ** applied))
    return torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8).cuda()


def launch(kind, d, table, rec=None):
    from dyk import lib as L
    fn = L.load().dyk_adam_step_groups if kind == "adam" else L.load().dyk_sgd_step_groups
    rc = fn(ctypes.byref(d), ctypes.byref(table) if table is not None else None,
            ctypes.c_void_p(rec.data_ptr()) if rec is not None else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def launch_existing(kind, d, rec=None):
    from dyk import lib as L
    h = L.load()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if rec is None:
        rc = (h.dyk_adam_step if kind == "adam" else h.dyk_sgd_step)(ctypes.byref(d), s)
    else:
        rc = (h.dyk_adam_step_guarded if kind == "adam" else h.dyk_sgd_step_guarded)(ctypes.byref(d), ctypes.c_void_p(rec.data_ptr()), s)
    torch.cuda.synchronize()
    return rc


def hyper(kind, step, grad_scale=1.0):
    return _h(**dict(SHARED[kind], grad_scale=grad_scale, step=step))


def desc(b, h, **kw):
    return b.desc(dict(IGNORED, **h), mask=True, **kw)


def check(kind, b, before, gmap, groups, h, planted=0, what=""):
    ref = R.grouped_step_ref(kind, before["p"], before["g"], before["m"], before["v"] if kind == "adam" else None, gmap, groups, **h)
    worst = [_within(b.get("p"), ref[0], ref[3], planted, what + " p"), _within(b.get("m"), ref[1], ref[4], planted, what + " m")]
    if kind == "adam":
        worst.append(_within(b.get("v"), ref[2], ref[5], planted, what + " v"))
    return worst


# ------------------------------------------------------------------ one step, every element, against fp64
def _one_step(kind, name, with_rec, step, grad_scale, zero_grad, wc):
    n, gmap, groups = layout(name, kind)
    h = hyper(kind, step, grad_scale)
    before = inputs(kind, n, 100 + step, h["beta1"], h["grad_scale"])
    b = Bufs(n, mask=gmap, **before)
    rec, eff = None, h
    if with_rec:                                            # step and grad_scale come from the record, the descriptor's step is 0
        coef = 0.75
        rec = record(h, step, coef)
        eff = dict(h, grad_scale=float(f32(h["grad_scale"]) * f32(coef)))
    keep = rec.clone() if with_rec else None
    assert launch(kind, desc(b, dict(h, step=0 if with_rec else step), zero_grad=zero_grad, wc=wc), table_of(groups), rec) == 0
    assert b.guards_intact()
    what = "%s %s rec %s step %d gs %g" % (kind, name, with_rec, step, grad_scale)
    worst = check(kind, b, before, gmap, groups, eff, what=what)
    if zero_grad:
        assert not b.bits("g").any(), "g must be +0.0 everywhere, frozen ranges included"
    else:
        assert np.array_equal(b.bits("g"), _i32(before["g"]))
    live = torch.from_numpy(gmap != 0)
    if wc:
        assert torch.equal(b.view("wc").cpu()[live], b.view("p").cpu().bfloat16().view(torch.int16)[live])
        assert np.all(b.bits("wc")[gmap == 0] == 0x1234)
    else:
        assert np.all(b.bits("wc") == 0x1234)
    if kind == "sgd":
        assert np.all(b.bits("v") == 0x7fc12345)
    assert np.array_equal(b.bits("mask"), gmap)
    if with_rec:
        assert torch.equal(rec, keep), "the step only reads the record"
    frozen = gmap == 0
    for k in ("p", "m") + (("v",) if kind == "adam" else ()):
        assert np.array_equal(b.bits(k)[frozen], _i32(before[k])[frozen]), k
    if n > 4:
        assert (b.bits("p") != _i32(before["p"]))[~frozen].mean() > 0.5
    return [round(w, 3) for w in worst]


@pytest.mark.parametrize("name", ["one", "interleaved"])
@pytest.mark.parametrize("with_rec", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_one_step_matches_fp64_within_the_derived_bound(kind, with_rec, name):
    worst = {}
    for step in (1, 2, 1000):
        for grad_scale in (1.0, 1 / 65536):
            zero_grad = int(step == 2)
            worst[(step, grad_scale)] = _one_step(kind, name, with_rec, step, grad_scale, zero_grad, wc=bool(zero_grad))
    print("%s %s rec %s: worst |got-ref|/bound (p, m[, v]) per (step, gs): %s" % (kind, name, with_rec, worst))
    assert max(max(w) for w in worst.values()) <= 1.0


@pytest.mark.parametrize("with_rec,step,grad_scale", [(False, 2, 1.0), (True, 1000, 1 / 65536)])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_second_ragged_sweep_with_group_changes_in_both_sweeps(kind, with_rec, step, grad_scale):
    worst = _one_step(kind, "big", with_rec, step, grad_scale, zero_grad=1, wc=True)
    print("%s big rec %s step %d gs %g: worst ratios %s" % (kind, with_rec, step, grad_scale, worst))
    assert max(worst) <= 1.0


def test_a_byte_above_the_count_is_frozen():
    n, gmap, groups = layout("interleaved", "adam")
    h = hyper("adam", 3)
    before = inputs("adam", n, 103, h["beta1"], 1.0)
    b = Bufs(n, mask=gmap, **before)
    assert launch("adam", desc(b, h, zero_grad=1), table_of(groups[:2])) == 0
    assert b.guards_intact()
    seen = np.where(gmap > 2, 0, gmap).astype(np.uint8)
    check("adam", b, before, seen, groups[:2], h)
    for k in ("p", "m", "v"):
        assert np.array_equal(b.bits(k)[gmap > 2], _i32(before[k])[gmap > 2]), k
    assert np.all(b.bits("wc")[gmap > 2] == 0x1234) and not b.bits("g").any()


# ------------------------------------------------------------------ the same bits as the plain and the _guarded entries
@pytest.mark.parametrize("name", ["interleaved", "big"])
@pytest.mark.parametrize("with_rec", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_equal_groups_give_the_bits_of_the_existing_kernels(kind, with_rec, name):
    """several groups with identical hyper-parameters and no decoupling == dyk_adam_step / dyk_sgd_step (with a record: the
    _guarded entries) with the mask binarised: p, m, v, wc, g and the guard bands, bit for bit"""
    n, gmap, _ = layout(name, kind)
    h = hyper(kind, 6, 1 / 8)
    one = dict(lr=1e-3, weight_decay=5e-4)
    before = inputs(kind, n, 44, h["beta1"], h["grad_scale"])
    rec = record(h, 6, 0.75) if with_rec else None
    a = Bufs(n, mask=gmap, **before)
    assert launch(kind, desc(a, dict(h, step=0 if with_rec else 6), zero_grad=1), table_of([one] * int(gmap.max())), rec) == 0
    b = Bufs(n, mask=(gmap != 0).astype(np.uint8), **before)
    assert launch_existing(kind, b.desc(dict(h, **_h(**one)), mask=True, zero_grad=1), rec) == 0
    assert a.guards_intact() and b.guards_intact()
    for k in ("p", "g", "m", "v", "wc"):
        assert torch.equal(a.full[k].view(torch.uint8), b.full[k].view(torch.uint8)), k
    assert not np.array_equal(a.bits("p"), _i32(before["p"]))


@pytest.mark.parametrize("with_rec", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_every_l2_group_of_a_mixed_launch_has_the_bits_of_the_existing_kernel(kind, with_rec):
    """group k of ONE mixed launch == the plain (with a record: the _guarded) entry launched with group k's lr / weight_decay and a
    mask that keeps group k only (one kernel template behind all entries: this is the ABI's contract).  The decoupled group has no
    counterpart; it must leave the others alone."""
    n, gmap, groups = layout("interleaved", kind)
    for step in (1, 1000):
        h = hyper(kind, step, 1 / 8)
        before = inputs(kind, n, 45, h["beta1"], h["grad_scale"])
        rec = record(h, step, 0.75) if with_rec else None
        a = Bufs(n, mask=gmap, **before)
        assert launch(kind, desc(a, dict(h, step=0 if with_rec else step), zero_grad=0), table_of(groups), rec) == 0
        assert a.guards_intact()
        for k, g in enumerate(groups, 1):
            if g.get("decoupled"):
                continue
            sel = gmap == k
            b = Bufs(n, mask=sel.astype(np.uint8), **before)
            hk = dict(h, **_h(lr=g["lr"], weight_decay=g["weight_decay"]))
            assert launch_existing(kind, b.desc(hk, mask=True, zero_grad=0), rec) == 0
            assert b.guards_intact()
            for name in ("p", "m", "v", "wc"):
                assert np.array_equal(a.bits(name)[sel], b.bits(name)[sel]), (name, k, step)
            assert (a.bits("p")[sel] != _i32(before["p"])[sel]).mean() > 0.5


# ------------------------------------------------------------------ sub-range launches (side stream, DDP buckets)
def _inside_each_group(gmap):
    """one cut (a multiple of 8) strictly inside a run of every group"""
    cuts = []
    for k in range(1, int(gmap.max()) + 1):
        idx = np.flatnonzero(gmap == k)
        mid = int(idx[len(idx) // 2 + 24]) // 8 * 8            # (runs are whole 64-element entries: 24 or 56 elements into one)
        assert mid > 0 and gmap[mid - 1] == k and gmap[mid] == k
        cuts.append(mid)
    return cuts


@pytest.mark.parametrize("name,cuts", [("interleaved", (8, 1000, 2048)), ("big", (BIG * 19 // 20 // 8 * 8,))])
@pytest.mark.parametrize("with_rec", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_sub_range_launches_are_bit_identical_to_one_launch(kind, with_rec, name, cuts):
    n, gmap, groups = layout(name, kind)
    h = hyper(kind, 6, 1 / 8)
    before = inputs(kind, n, 44, h["beta1"], h["grad_scale"])
    rec = record(h, 6, 0.75) if with_rec else None
    t = table_of(groups)
    hd = dict(h, step=0 if with_rec else 6)
    whole = Bufs(n, mask=gmap, **before)
    assert launch(kind, desc(whole, hd, zero_grad=1), t, rec) == 0
    parts = Bufs(n, mask=gmap, **before)
    edges = sorted({0, n} | set(cuts) | set(_inside_each_group(gmap)))
    assert all(c % 8 == 0 for c in edges[:-1]) and len(edges) >= len(cuts) + len(groups) + 2
    for lo, hi in reversed(list(zip(edges, edges[1:]))):
        assert launch(kind, desc(parts, hd, zero_grad=1, off=lo, cnt=hi - lo), t, rec) == 0
    assert whole.guards_intact() and parts.guards_intact()
    for k in whole.full:
        assert torch.equal(whole.full[k].view(torch.uint8), parts.full[k].view(torch.uint8)), k
    assert not torch.equal(whole.view("p"), torch.from_numpy(before["p"]).cuda())


# ------------------------------------------------------------------ the bf16 copy
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bf16_copy_is_the_round_to_nearest_even_of_the_stored_fp32_on_live_elements(kind):
    """lr = 0, wd = 0 (decay_mul = 1), g = 0, m = 0, v = 1 in every group: p passes through, and wc shows the hardware conversion
    of chosen bit patterns on live elements; frozen entries keep their old copy"""
    n, gmap, groups = layout("interleaved", kind)
    groups = [dict(g, lr=0.0, weight_decay=0.0) for g in groups]
    assert all(r[2] == 1.0 for r in R.table(groups))
    h = hyper(kind, 1)
    p = _bf16_specials(n)
    z = np.zeros(n, np.float32)
    b = Bufs(n, mask=gmap, p=p, g=z, m=z, v=np.ones(n, np.float32))
    assert launch(kind, desc(b, h), table_of(groups)) == 0
    assert b.guards_intact()
    live = gmap != 0
    p_after = b.view("p").cpu()
    nan = torch.isnan(p_after)
    assert torch.equal(nan, torch.from_numpy(np.isnan(p)))
    ok = ~nan.numpy()
    assert np.array_equal(b.bits("p")[ok], _i32(p)[ok]), "p * 1 - 0 must be p (denormals and -0 included)"
    assert np.array_equal(b.bits("p")[~live], _i32(p)[~live])
    wc = b.view("wc").cpu()
    want = p_after.bfloat16().view(torch.int16)
    sel = torch.from_numpy(live) & ~nan
    assert torch.equal(wc[sel], want[sel])
    assert torch.equal(torch.isnan(wc.view(torch.bfloat16))[torch.from_numpy(live)], nan[torch.from_numpy(live)])
    assert np.all(b.bits("wc")[~live] == 0x1234)
    got = wc.view(torch.bfloat16).float()[torch.from_numpy(live)]
    assert int(torch.isinf(got).sum()) > int(torch.isinf(p_after[torch.from_numpy(live)]).sum())   # finite values did round up to Inf


# ------------------------------------------------------------------ a record with skip = 1
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_skipping_record_leaves_p_m_v_wc_and_clears_g_when_asked(kind, zero_grad):
    n, gmap, groups = layout("interleaved", kind)
    h = hyper(kind, 0)
    before = inputs(kind, n, 46, h["beta1"], 1.0)
    b = Bufs(n, mask=gmap, **before)
    snap = b.snapshot()
    assert launch(kind, desc(b, h, zero_grad=zero_grad), table_of(groups), record(h, 3, 0.75, skip=1)) == 0
    now = b.snapshot()
    for k in ("p", "m", "v", "wc", "mask"):
        assert np.array_equal(now[k], snap[k]), k
    if zero_grad:
        assert not b.bits("g").any() and b.guards_intact()
    else:
        assert np.array_equal(now["g"], snap["g"])


# ------------------------------------------------------------------ non-finite gradients stay in their own lane
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_non_finite_gradients_poison_only_their_own_element(kind):
    n, gmap, groups = layout("interleaved", kind)
    h = hyper(kind, 5)
    before = {k: a.copy() for k, a in inputs(kind, n, 21, h["beta1"], 1.0).items()}
    planted = np.array([1, 64 + 2, 64 * (len(groups) - 1) + 7])            # three groups (the last one included), three lane positions
    assert len(set(gmap[planted])) == 3 and gmap[planted].min() > 0 and len(set(planted % 4)) == 3
    before["g"][planted] = np.array([np.nan, np.inf, -np.inf], np.float32)
    b = Bufs(n, mask=gmap, **before)
    assert launch(kind, desc(b, h), table_of(groups)) == 0
    assert b.guards_intact()
    check(kind, b, before, gmap, groups, h, planted=3)
    for k in ("p", "m") + (("v",) if kind == "adam" else ()):
        assert np.array_equal(np.flatnonzero(~np.isfinite(b.get(k))), planted), k


# ------------------------------------------------------------------ argument checks: nothing is written
BAD = ["mask_null", "count_0", "count_9", "count_negative", "wd_negative", "wd_nan", "lr_nan", "lr_inf", "mask_misaligned",
       "unknown_flag", "groups_null", "step_zero", "rec_misaligned", "n_not_4", "p_null", "v_misaligned"]


@pytest.mark.parametrize("bad", BAD + ["decoupled"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bad_arguments_are_rejected_and_write_nothing(kind, bad):
    n, gmap, groups = 256, R.interleaved_map(256, 3, 0), L2
    h = hyper(kind, 2)
    before = inputs(kind, n, 55, h["beta1"], 1.0)
    b = Bufs(n, mask=gmap, **before)
    d = desc(b, h, zero_grad=1)
    t = table_of(groups)
    rec = None
    want = ERR_ARG
    if bad == "mask_null":
        d.mask = None
    elif bad.startswith("count_"):
        t.count = {"0": 0, "9": 9, "negative": -1}[bad.split("_")[1]]
    elif bad == "wd_negative":
        t.g[1].weight_decay = -1e-4
    elif bad == "wd_nan":
        t.g[2].weight_decay = float("nan")
    elif bad == "lr_nan":
        t.g[2].lr = float("nan")
    elif bad == "lr_inf":
        t.g[0].lr = float("inf")
    elif bad == "mask_misaligned":
        d.mask, d.n = d.mask + 2, n - 8
    elif bad == "unknown_flag":
        t.g[0].flags = 2
    elif bad == "groups_null":
        t = None
    elif bad == "step_zero":
        d.step = 0
    elif bad == "rec_misaligned":
        rec = torch.zeros(48, dtype=torch.uint8, device="cuda")[4:44]          # 4 bytes off the 8-byte alignment
    elif bad == "n_not_4":
        d.n = n - 2
    elif bad == "p_null":
        d.p = None
    elif bad == "v_misaligned":
        d.v, d.n = d.v + 8, n - 8
    elif bad == "decoupled":
        t.g[1].flags = 1
        want = 0 if kind == "adam" else ERR_UNSUPPORTED
    snap = b.snapshot()
    rc = launch(kind, d, t, rec)
    assert rc == want
    now = b.snapshot()
    if want == 0:                                           # (a decoupled group is Adam's to take)
        assert b.guards_intact() and not np.array_equal(now["p"], snap["p"])
        return
    for k in snap:
        assert np.array_equal(now[k], snap[k]), k
