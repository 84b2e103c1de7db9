"""The gradient guard of csrc/optim_guard.hip at its own ABI, through dyk/ops.py, on plain CUDA tensors (no model):
dyk_grad_stats against a plain fp64 norm (and, bit for bit, against the numpy restatement of its reduction order in
tests/grad_guard_ref.py), the clip coefficient, dyk_adam_step_guarded / dyk_sgd_step_guarded per element against the fp64
reference of oracle/optim.py and bit for bit against dyk_adam_step / dyk_sgd_step, skipped steps, dyk_grad_scale_by_rec and the
argument checks.  Inputs: oracle.optim.input_family; buffers and per-element checks: the ones of tests/test_gpu_optim.py."""
import numpy as np
import pytest
import torch

import grad_guard_ref as R
from oracle.optim import input_family
from test_gpu_optim import ADAM, SGD, Bufs, _check_step, _family, _h, _i32

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -23          # |norm - ref| <= 2^-23 * ref: derived in tests/grad_guard_ref.py (fp64 accumulation, one fp32 rounding)
N_MASKED = 65540
N_FULL = R.first_full_n()
GS = 1 / 8
_CACHE = {}


def _case(n, masked):
    """(g, mask, fp64 norm of fl32(g * GS) over the live elements), computed once per process and shared (do not modify)"""
    key = (n, masked)
    if key not in _CACHE:
        g = input_family(n, n % 97)[1]
        mask = R.entry_mask(n) if masked else None
        _CACHE[key] = (g, mask, R.plain_reference(g, mask, GS)[0])
    return _CACHE[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(g, mask, rec=None, **kw):
    """one dyk_grad_stats call on device tensors -> (record struct, raw record bytes, record tensor)"""
    from dyk import ops
    n = g.numel()
    rec = ops.grad_guard_record(g.device) if rec is None else rec
    need = int(ops.load().dyk_grad_stats_ws_bytes(n))
    big = torch.full((need + 64,), 0xa5, dtype=torch.uint8, device=g.device)
    ops.grad_stats(g, rec, big[:need], mask=mask, **kw)
    torch.cuda.synchronize()
    assert bool((big[need:] == 0xa5).all()), "the partials kernel wrote past its workspace"
    raw = rec.cpu().numpy().tobytes()
    return ops.grad_record_from_bytes(raw), raw, rec


def _f32bits(x):
    return np.float32(x).view(np.uint32)


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize("n,masked", [(4, False), (1028, False), (N_MASKED, True), (N_FULL, False)])
def test_norm_and_count_against_fp64(n, masked):
    from dyk import ops
    g, mask, ref = _case(n, masked)
    assert int(ops.load().dyk_grad_stats_ws_bytes(n)) == 16 * R.grid_blocks(n)
    gd, md = _dev(g), _dev(mask)
    r1, raw1, _ = _stats(gd, md, grad_scale=GS, beta1=0.937, beta2=0.999)
    r2, raw2, _ = _stats(gd, md, grad_scale=GS, beta1=0.937, beta2=0.999)
    print("n %d: norm %.9g ref %.17g rel err %.3g (bound %.3g)" % (n, r1.norm, ref, abs(r1.norm - ref) / ref, BOUND))
    assert abs(float(r1.norm) - ref) <= BOUND * ref
    assert r1.nonfinite == 0 and r1.skip == 0 and r1.applied == 1 and r1.skipped == 0 and r1.coef == 1.0
    assert raw1 == raw2, "two runs of the same reduction differ"
    # the documented order, bit for bit
    want = R.stats(R.new_record(), g, mask, grad_scale=GS, beta1=0.937, beta2=0.999)
    assert np.float64(r1.sumsq).view(np.uint64) == np.float64(want["sumsq"]).view(np.uint64)
    assert _f32bits(r1.norm) == _f32bits(want["norm"])
    assert _f32bits(r1.bc1) == _f32bits(want["bc1"]) and _f32bits(r1.bc2_sqrt) == _f32bits(want["bc2_sqrt"])
    assert torch.equal(gd.cpu(), torch.from_numpy(g))


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("n", [1028, N_FULL])
def test_planted_non_finite_values_are_counted(n, value):
    g, _, _ = _case(n, False)
    T = R.grid_blocks(n) * R.BLOCK                         # threads of the grid: vector T starts the second sweep
    spots = sorted({0, n - 1} | ({4 * T - 1, 4 * T} if 4 * T < n else {4 * (n // 8) - 1, 4 * (n // 8)}))
    a = g.copy()
    a[spots] = value
    for skip in (False, True):
        r, _, _ = _stats(_dev(a), None, grad_scale=GS, skip_nonfinite=skip)
        assert r.nonfinite == len(spots) == 4
        assert r.skip == int(skip) and r.applied == int(not skip) and r.skipped == int(skip)
        assert not np.isfinite(r.norm)
    # one at a time: every position on its own
    for s in spots:
        b = g.copy()
        b[s] = value
        assert _stats(_dev(b), None, grad_scale=GS)[0].nonfinite == 1, s


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
def test_values_under_mask_0_are_not_counted(value):
    g, mask, ref = _case(N_MASKED, True)
    frozen = np.flatnonzero(mask == 0)
    assert frozen[0] == 0 and frozen[-1] == N_MASKED - 1
    a = g.copy()
    a[[frozen[0], frozen[-1], frozen[len(frozen) // 2], frozen[63], frozen[64]]] = value
    r, _, _ = _stats(_dev(a), _dev(mask), grad_scale=GS, skip_nonfinite=True)
    assert r.nonfinite == 0 and r.skip == 0 and r.applied == 1
    assert abs(float(r.norm) - ref) <= BOUND * ref
    # ... and the same values are counted without the mask
    assert _stats(_dev(a), None, grad_scale=GS)[0].nonfinite == 5


def test_clip_coefficient():
    g, mask, ref = _case(N_MASKED, True)
    gd, md = _dev(g), _dev(mask)
    f = np.float32
    r, _, _ = _stats(gd, md, grad_scale=GS, max_norm=0.5 * ref)
    want = f(0.5 * ref) / (f(r.norm) + f(1e-6))
    assert _f32bits(r.coef) == _f32bits(want) and 0.49 < r.coef < 0.51
    r, _, _ = _stats(gd, md, grad_scale=GS, max_norm=2 * ref)
    assert r.coef == 1.0
    r, _, _ = _stats(gd, md, grad_scale=GS, max_norm=0.0)
    assert r.coef == 1.0
    a = g.copy()
    a[100] = np.nan                                         # live
    r, _, _ = _stats(_dev(a), md, grad_scale=GS, max_norm=1.0)
    assert np.isnan(r.coef) and np.isnan(r.norm) and r.nonfinite == 1 and r.skip == 0


# ------------------------------------------------------------------ guarded steps
def _hyper(kind, **kw):
    return _h(**dict(ADAM if kind == "adam" else SGD, grad_scale=GS, **kw))


def _guarded(kind, b, d, rec):
    from dyk import ops
    (ops.adam_step_guarded if kind == "adam" else ops.sgd_step_guarded)(d, rec)
    torch.cuda.synchronize()
    assert b.guards_intact()


def _plain(kind, b, d):
    import ctypes
    from dyk import lib as L
    fn = L.load().dyk_adam_step if kind == "adam" else L.load().dyk_sgd_step
    assert fn(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert b.guards_intact()


def _stats_for(b, h, rec, mask, **kw):
    betas = dict(beta1=h["beta1"], beta2=h["beta2"]) if h.get("beta2") else {}
    return _stats(b.view("g"), b.view("mask") if mask is not None else None, rec, grad_scale=h["grad_scale"], **betas, **kw)[0]


def _state(b):
    return {k: b.get(k) for k in ("p", "g", "m", "v")}


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_three_guarded_steps_against_fp64_and_the_plain_kernels(kind, clip):
    """every step: p, m, v per element within the bound of oracle/optim.py for grad_scale = fl32(gs * coef) as read back from the
    record and step = applied.  Without clipping the guarded kernel must also reproduce dyk_adam_step / dyk_sgd_step bit for
    bit (p, m, v, wc, g): same statements, coef = 1, the same bias corrections."""
    from dyk import ops
    n = N_MASKED
    mask = R.entry_mask(n)
    h = _hyper(kind)
    first = _family(kind, n, 300, dict(h))
    b = Bufs(n, mask=mask, **first)
    twin = Bufs(n, mask=mask, **first)
    rec = ops.grad_guard_record("cuda")
    f = np.float32
    worst = []
    for step in (1, 2, 3):
        g = input_family(n, 300 + step, kind, h["beta1"], GS)[1]
        b.set(g=g)
        twin.set(g=g)
        before = _state(b)
        ref_norm = R.plain_reference(g, mask, GS)[0]
        r = _stats_for(b, h, rec, mask, max_norm=0.5 * ref_norm if clip else 0.0, skip_nonfinite=True)
        assert r.applied == step and r.skip == 0 and r.skipped == 0
        assert (0.49 < r.coef < 0.51) if clip else r.coef == 1.0
        _guarded(kind, b, b.desc(dict(h, step=0), mask=True, zero_grad=1), rec)
        eff = dict(h, grad_scale=float(f(h["grad_scale"]) * f(r.coef)), step=r.applied)
        worst.append([round(w, 3) for w in _check_step(kind, b, before, eff, mask, what="%s step %d" % (kind, step))])
        assert not b.bits("g").any()
        assert torch.equal(b.view("wc").cpu()[mask == 1], b.view("p").cpu().bfloat16().view(torch.int16)[mask == 1])
        assert np.all(b.bits("wc")[mask == 0] == 0x1234)
        if not clip:
            _plain(kind, twin, twin.desc(dict(h, step=step), mask=True, zero_grad=1))
            for k in b.full:
                assert torch.equal(b.full[k].view(torch.uint8), twin.full[k].view(torch.uint8)), (k, step)
    print("%s clip %s: worst |got-ref|/bound per step %s" % (kind, clip, worst))
    assert max(max(w) for w in worst) <= 1.0


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_guarded_sub_range_launches_read_one_record(kind, use_mask):
    """the two ranges of dyk.optim._FusedBase._launch: statistics over the whole buffer, then [lo, n) and [0, lo) separately"""
    from dyk import ops
    n = N_MASKED
    mask = R.entry_mask(n)
    h = _hyper(kind)
    first = _family(kind, n, 44, dict(h))
    whole, parts = Bufs(n, mask=mask, **first), Bufs(n, mask=mask, **first)
    lo = n * 19 // 20 // 8 * 8
    for b, ranges in ((whole, [(0, n)]), (parts, [(lo, n), (0, lo)])):
        rec = ops.grad_guard_record("cuda")
        r = _stats_for(b, h, rec, mask if use_mask else None, max_norm=0.5 * R.plain_reference(first["g"], mask if use_mask else None, GS)[0])
        assert r.applied == 1 and r.coef < 1
        for a, e in ranges:
            _guarded(kind, b, b.desc(dict(h, step=0), mask=use_mask, zero_grad=1, off=a, cnt=e - a), rec)
    for k in whole.full:
        assert torch.equal(whole.full[k].view(torch.uint8), parts.full[k].view(torch.uint8)), k
    assert not np.array_equal(whole.bits("p"), _i32(first["p"]))


# ------------------------------------------------------------------ skipped steps
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("poison_first", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_poisoned_step_is_skipped_and_does_not_advance_the_step_count(kind, poison_first, zero_grad):
    """steps 1..3 with an inf planted before step 2 (and, poison_first, before step 1 as well): the poisoned step leaves p, m, v,
    wc bit for bit; the next clean step is the reference's step `applied` from that state -- Adam's bias correction at t = 2,
    SGD's first-step rule (m = g') exactly at the first APPLIED step."""
    from dyk import ops
    n = N_MASKED
    mask = R.entry_mask(n)
    live = np.flatnonzero(mask)
    h = _hyper(kind)
    b = Bufs(n, mask=mask, **_family(kind, n, 400, dict(h)))
    rec = ops.grad_guard_record("cuda")
    poisoned = {1, 2} if poison_first else {2}
    applied = skipped = 0
    for step in (1, 2, 3):
        g = input_family(n, 400 + step, kind, h["beta1"], GS)[1]
        if step in poisoned:
            g = g.copy()
            g[live[len(live) // 3]] = np.inf
        b.set(g=g)
        before = _state(b)
        snap = b.snapshot()
        r = _stats_for(b, h, rec, mask, skip_nonfinite=True)
        _guarded(kind, b, b.desc(dict(h, step=0), mask=True, zero_grad=zero_grad), rec)
        if step in poisoned:
            skipped += 1
            assert r.skip == 1 and r.nonfinite == 1
            now = b.snapshot()
            for k in ("p", "m", "v", "wc", "mask"):
                assert np.array_equal(now[k], snap[k]), (k, step)
            if zero_grad:
                assert not b.bits("g").any(), "g must be cleared on a skipped step too (frozen ranges included)"
            else:
                assert np.array_equal(now["g"], snap["g"])
        else:
            applied += 1
            assert r.skip == 0 and r.nonfinite == 0
            _check_step(kind, b, before, dict(h, step=applied), mask, what="%s step %d as t=%d" % (kind, step, applied))
            if kind == "sgd" and applied == 1:
                # the first-step rule fired: m' = g' -- not mom*m + g' (the family's m is far from 0)
                gr = before["g"].astype(np.float64) * h["grad_scale"] + h["weight_decay"] * before["p"].astype(np.float64)
                sel = (mask == 1) & (np.abs(before["m"]) > 1e-3)
                assert sel.sum() > 1000 and np.allclose(b.get("m")[sel], gr[sel], rtol=1e-5, atol=1e-30)
        assert (r.applied, r.skipped) == (applied, skipped)
    assert (applied, skipped) == ((1, 2) if poison_first else (2, 1))


# ------------------------------------------------------------------ stand-alone scaling (dyk.optim.clip_grad_norm_)
def test_grad_scale_by_rec():
    from dyk import ops
    g, mask, ref = _case(N_MASKED, True)
    gd, md = _dev(g), _dev(mask)
    r, _, rec = _stats(gd, md, max_norm=0.5 * R.plain_reference(g, mask, 1.0)[0])
    assert 0.49 < r.coef < 0.51
    ops.grad_scale_by_rec(gd, rec, mask=md)
    torch.cuda.synchronize()
    got = gd.cpu().numpy()
    want = np.where(mask == 1, g * np.float32(r.coef), g)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[mask == 1], g[mask == 1])
    # coef == 1: nothing is stored (a pattern that a multiplication by 1 would not keep: signalling NaNs become quiet)
    odd = g.copy()
    odd.view(np.uint32)[200:204] = 0x7fa00001
    od = _dev(odd)
    rec1 = ops.grad_guard_record("cuda")
    r1, _, _ = _stats(_dev(g), md, rec1, max_norm=0.0)
    assert r1.coef == 1.0
    ops.grad_scale_by_rec(od, rec1, mask=md)
    torch.cuda.synchronize()
    assert np.array_equal(od.cpu().numpy().view(np.uint32), odd.view(np.uint32))
    # without a mask every element is scaled
    gd2 = _dev(g)
    ops.grad_scale_by_rec(gd2, rec, mask=None)
    torch.cuda.synchronize()
    assert np.array_equal(gd2.cpu().numpy().view(np.uint32), (g * np.float32(r.coef)).view(np.uint32))


# ------------------------------------------------------------------ argument checks
def test_bad_arguments_are_rejected_before_any_launch():
    from dyk import ops
    from dyk.lib import DykError
    n = 1028
    g = _dev(_case(n, False)[0])
    keep = g.clone()
    rec = ops.grad_guard_record("cuda")
    ws = ops.grad_stats_workspace(n, "cuda")
    err = r"\(-1\)"                                          # DYK_ERR_ARG
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g, rec, ws, n=6)
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g[1:n - 3], rec, ws)                  # g off by 4 bytes
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g, None, ws)                          # null record
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g, rec, ws[:ws.numel() - 1])          # workspace one byte short
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g, rec, None)
    with pytest.raises(DykError, match=err):
        ops.grad_stats(g, rec[4:], torch.empty(64, dtype=torch.uint8, device="cuda"), n=4)     # record off by 4 bytes
    with pytest.raises(DykError, match=err):
        ops.grad_scale_by_rec(g, rec, n=6)
    with pytest.raises(DykError, match=err):
        ops.grad_scale_by_rec(g[1:n - 3], rec)
    with pytest.raises(DykError, match=err):
        ops.grad_scale_by_rec(g, None)
    for kind in ("adam", "sgd"):
        h = _hyper(kind, step=0)
        b = Bufs(256, **_family(kind, 256, 55, dict(h)))
        snap = b.snapshot()
        step = ops.adam_step_guarded if kind == "adam" else ops.sgd_step_guarded
        bad_n = b.desc(h, mask=True, zero_grad=1)
        bad_n.n = 6
        off4 = b.desc(h, mask=True, zero_grad=1)
        off4.g, off4.n = off4.g + 4, 252
        for d, r in ((bad_n, rec), (off4, rec), (b.desc(h, mask=True, zero_grad=1), None)):
            with pytest.raises(DykError, match=err):
                step(d, r)
        torch.cuda.synchronize()
        now = b.snapshot()
        for k in snap:
            assert np.array_equal(now[k], snap[k]), k
    torch.cuda.synchronize()
    assert torch.equal(g, keep) and not bool(rec.any())
