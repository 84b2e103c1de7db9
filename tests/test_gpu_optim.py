"""dyk_adam_step / dyk_sgd_step (csrc/optim.hip) at their own ABI: DykOptimDesc built by hand over plain CUDA tensors, no model.
Every element of p, m, v is held to the fp64 reference of oracle/optim.py within its derived bound (tests/test_optim_reference.py
shows what that bound lets through and what it catches); the bf16 copy, the gradient clearing, the frozen-parameter mask, the
sub-range launches of the side stream / DDP buckets and the argument checks are compared bit for bit.  Every buffer sits between
guard bands that are checked after each launch."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import OPTIM_K
from oracle.optim import adam_step_ref, input_family, sgd_step_ref

pytestmark = pytest.mark.gpu

GUARD = 64                                     # elements on either side of every buffer (keeps the 16 / 8 / 4 byte alignments)
GUARD_BITS = {torch.float32: 0x7fa5a5a5, torch.int16: 0x5a5a, torch.uint8: 0xa5}
BIG = 8192 * 256 * 4 + 4 * 257                 # 8192 blocks x 256 threads x float4 cover the first sweep; the second one is ragged
STEPS = (1, 2, 10, 1000, 100000)
ERR_ARG = -1                                   # DYK_ERR_ARG (include/dyk_hip.h)


def _h(**kw):
    """hyper-parameters as the descriptor carries them (c_float rounds to fp32)"""
    return {k: (v if k == "step" else float(np.float32(v))) for k, v in kw.items()}


ADAM = dict(lr=1e-3, beta1=0.937, beta2=0.999, eps=1e-8, weight_decay=5e-4, grad_scale=1.0)
SGD = dict(lr=1e-2, beta1=0.937, beta2=0.0, eps=0.0, weight_decay=5e-4, grad_scale=1.0)


class Bufs:
    """p, g, m, v (fp32), wc (bf16 as int16), mask (bytes) on the device, each inside guard bands"""
    dtypes = dict(p=torch.float32, g=torch.float32, m=torch.float32, v=torch.float32, wc=torch.int16, mask=torch.uint8)

    def __init__(self, n, **arrays):
        self.n = n
        self.full = {}
        for k, dt in self.dtypes.items():
            if dt == torch.float32:
                t = torch.full((n + 2 * GUARD,), GUARD_BITS[dt], dtype=torch.int32, device="cuda").view(torch.float32)
            else:
                t = torch.full((n + 2 * GUARD,), GUARD_BITS[dt], dtype=dt, device="cuda")
            self.full[k] = t
        self.set(**dict(dict(wc=np.full(n, 0x1234, np.int16), mask=np.ones(n, np.uint8)), **arrays))

    def view(self, k):
        return self.full[k][GUARD:GUARD + self.n]

    def set(self, **arrays):
        for k, a in arrays.items():
            self.view(k).copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def bits(self, k, full=False):
        t = self.full[k] if full else self.view(k)
        return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu().numpy().copy()

    def get(self, k):
        return self.view(k).cpu().numpy().copy()

    def snapshot(self):
        return {k: self.bits(k, full=True) for k in self.full}

    def guards_intact(self):
        for k, t in self.full.items():
            raw = t.view(torch.int32) if t.dtype == torch.float32 else t
            want = GUARD_BITS[self.dtypes[k]]
            if not (bool((raw[:GUARD] == want).all()) and bool((raw[GUARD + self.n:] == want).all())):
                return False
        return True

    def desc(self, h, wc=True, mask=False, v=True, zero_grad=0, off=0, cnt=None):
        """descriptor of [off, off + cnt) with the pointer arithmetic of dyk.optim._FusedBase._launch.sub"""
        from dyk import lib as L
        d = L.DykOptimDesc()
        base = {k: self.view(k).data_ptr() for k in self.full}
        d.p, d.g, d.m = base["p"] + 4 * off, base["g"] + 4 * off, base["m"] + 4 * off
        d.v = base["v"] + 4 * off if v else None
        d.mask = base["mask"] + off if mask else None
        d.wc = base["wc"] + 2 * off if wc else None
        d.n = self.n - off if cnt is None else cnt
        d.lr, d.beta1, d.beta2, d.eps = h["lr"], h["beta1"], h.get("beta2", 0.0), h.get("eps", 0.0)
        d.weight_decay, d.grad_scale, d.step, d.zero_grad = h["weight_decay"], h["grad_scale"], h["step"], zero_grad
        return d


def _fn(kind):
    from dyk import lib as L
    h = L.load()
    return h.dyk_adam_step if kind == "adam" else h.dyk_sgd_step


def _launch(kind, d):
    rc = _fn(kind)(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _reference(kind, p, g, m, v, mask, h):
    if kind == "adam":
        return adam_step_ref(p, g, m, v, mask, **h)
    return sgd_step_ref(p, g, m, v, mask, **h)


def _within(got, ref, bound, planted=0, what=""):
    """EVERY element: |got - ref| <= bound where the reference is finite; where it is not (at most `planted` elements), the same
    class (NaN, +Inf, -Inf).  -> worst |got - ref| / bound"""
    got = got.astype(np.float64)
    odd = ~np.isfinite(ref)
    assert int(odd.sum()) <= planted, (what, int(odd.sum()), planted)
    assert np.array_equal(~np.isfinite(got), odd), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[odd & ~np.isnan(ref)], ref[odd & ~np.isnan(ref)]), what
    ok = ~odd
    assert np.isfinite(bound[ok]).all(), what
    err = np.abs(got[ok] - ref[ok])
    bad = err > bound[ok]
    assert not bad.any(), "%s: %d of %d elements beyond the bound, worst ratio %.3g" % (
        what, int(bad.sum()), err.size, float(np.max(err[bad] / np.maximum(bound[ok][bad], 1e-300))))
    return float(np.max(np.where(err > 0, err / np.where(bound[ok] > 0, bound[ok], 1.0), 0.0))) if err.size else 0.0


def _check_step(kind, b, before, h, mask=None, planted=0, what=""):
    """p, m (and v for Adam) of `b` after one launch against the reference of the inputs `before`"""
    ref = _reference(kind, before["p"], before["g"], before["m"], before["v"], mask, h)
    worst = [_within(b.get("p"), ref[0], ref[3], planted, what + " p"), _within(b.get("m"), ref[1], ref[4], planted, what + " m")]
    if kind == "adam":
        worst.append(_within(b.get("v"), ref[2], ref[5], planted, what + " v"))
    return worst


def _family(kind, n, seed, h):
    p, g, m, v = input_family(n, seed, kind, h["beta1"], h["grad_scale"])
    return dict(p=p, g=g, m=m, v=v)


def _i32(a):
    return a.view(np.int32)


# ------------------------------------------------------------------ one step, every element, against fp64
@pytest.mark.parametrize("grad_scale", [1.0, 1 / 8, 1 / 65536])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("betas", [(0.937, 0.999), (0.5, 0.9)])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_one_step_matches_fp64_within_the_derived_bound(kind, betas, wd, grad_scale):
    """(0.5, 0.9) is deliberately asymmetric: swapped betas cannot hide behind it.  For SGD beta1 is the momentum and v is
    poisoned with NaN: the kernel must neither read nor write it."""
    n = 1 << 18
    worst = {}
    for step in STEPS:
        h = _h(**dict(ADAM if kind == "adam" else SGD, beta1=betas[0], weight_decay=wd, grad_scale=grad_scale, step=step))
        if kind == "adam":
            h["beta2"] = float(np.float32(betas[1]))
        before = _family(kind, n, 100 + step, h)
        if kind == "sgd":
            before["v"] = np.full(n, np.nan, np.float32)
            _i32(before["v"])[:] = 0x7fc12345
        b = Bufs(n, **before)
        assert _launch(kind, b.desc(h, wc=False)) == 0
        assert b.guards_intact()
        worst[step] = [round(r, 3) for r in _check_step(kind, b, before, h, what="%s step %d" % (kind, step))]
        assert np.array_equal(b.bits("g"), _i32(before["g"]))                    # zero_grad = 0
        assert np.all(b.bits("wc") == 0x1234)                                    # wc == NULL
        if kind == "sgd":
            assert np.all(b.bits("v") == 0x7fc12345)
    print("%s betas %s wd %g gs %g: worst |got-ref|/bound (p, m[, v]) per step: %s" % (kind, betas, wd, grad_scale, worst))
    assert max(max(w) for w in worst.values()) <= 1.0


def test_sgd_runs_without_a_second_moment_buffer():
    h = _h(**dict(SGD, step=3))
    before = _family("sgd", 3076, 7, h)
    b = Bufs(3076, **before)
    keep = b.bits("v")
    assert _launch("sgd", b.desc(h, v=False)) == 0
    assert b.guards_intact() and np.array_equal(b.bits("v"), keep)
    _check_step("sgd", b, before, h)


# ------------------------------------------------------------------ sizes: one vector ... a second, ragged grid-stride sweep
@pytest.mark.parametrize("n", [4, 64, 1024 * 3 + 4, BIG])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_sizes_up_to_a_second_grid_stride_sweep(kind, n):
    h = _h(**dict(ADAM if kind == "adam" else SGD, grad_scale=1 / 8, step=10))
    before = _family(kind, n, n % 1000, h)
    b = Bufs(n, **before)
    assert _launch(kind, b.desc(h, zero_grad=1)) == 0
    assert b.guards_intact()
    worst = _check_step(kind, b, before, h, what="%s n %d" % (kind, n))
    print("%s n %d: worst ratios %s" % (kind, n, [round(w, 3) for w in worst]))
    assert not b.bits("g").any()                                                 # all +0.0
    p_after = b.view("p").cpu()
    assert torch.equal(b.view("wc").cpu(), p_after.bfloat16().view(torch.int16))


# ------------------------------------------------------------------ the bf16 copy
def _bf16_specials(n):
    """fp32 bit patterns: random ones, and at every 5th element a case of the f32 -> bf16 rounding"""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([
        0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,      # exactly halfway: even / odd lower neighbour, both signs
        0x3f808001, 0x3f807fff, 0x3f818001, 0x3f817fff,      # just beside halfway
        0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00001, 0x7f800001,     # +-Inf, quiet / signalling NaN
        0x00000001, 0x007fffff, 0x80012345, 0x00008000, 0x00018000, 0x00400000,     # denormals (halfway ones included)
        0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,      # round up to +-Inf; the last one stays finite
        0x00000000, 0x80000000], dtype=np.uint32)
    pick = np.arange(0, n, 5)
    bits[pick] = special[np.arange(len(pick)) % len(special)]
    return bits.view(np.float32)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bf16_copy_is_the_round_to_nearest_even_of_the_stored_fp32(kind):
    """lr = 0, wd = 0, g = 0, m = 0, v = 1: the update is p - 0 * 0, p passes through, and wc shows the hardware conversion on
    chosen bit patterns.  The expected bits are torch's CPU conversion of the fp32 the kernel itself stored."""
    n = 1024 * 3 + 4
    h = _h(**dict(ADAM if kind == "adam" else SGD, lr=0.0, weight_decay=0.0, step=1))
    p = _bf16_specials(n)
    z = np.zeros(n, np.float32)
    b = Bufs(n, p=p, g=z, m=z, v=np.ones(n, np.float32))
    assert _launch(kind, b.desc(h)) == 0
    assert b.guards_intact()
    p_after = b.view("p").cpu()
    nan = torch.isnan(p_after)
    assert torch.equal(nan, torch.from_numpy(np.isnan(p)))
    assert np.array_equal(b.bits("p")[~nan.numpy()], _i32(p)[~nan.numpy()]), "p - 0 must be p (denormals and -0 included)"
    wc = b.view("wc").cpu()
    want = p_after.bfloat16()
    assert torch.equal(torch.isnan(wc.view(torch.bfloat16)), nan)
    assert torch.equal(wc[~nan], want.view(torch.int16)[~nan])
    got = wc.view(torch.bfloat16).float()
    assert int(torch.isinf(got).sum()) > int(torch.isinf(p_after).sum())         # some finite values did round up to Inf
    assert not b.bits("m").any() and not b.bits("g").any()


# ------------------------------------------------------------------ non-finite gradients stay in their own lane
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_non_finite_gradients_poison_only_their_own_element(kind):
    n = 4096
    h = _h(**dict(ADAM if kind == "adam" else SGD, step=5))
    before = _family(kind, n, 21, h)
    planted = np.arange(1, n, 4 * 37 + 1)                       # one lane of a float4 each, every lane position occurs
    assert len(set(planted // 4)) == len(planted) and set(planted % 4) == {0, 1, 2, 3}
    before["g"][planted] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(planted)) % 3]
    b = Bufs(n, **before)
    assert _launch(kind, b.desc(h)) == 0
    assert b.guards_intact()
    _check_step(kind, b, before, h, planted=len(planted))
    for k in ("p", "m") + (("v",) if kind == "adam" else ()):
        assert np.array_equal(np.flatnonzero(~np.isfinite(b.get(k))), planted), k
    # wc follows the stored p here too
    p_after = b.view("p").cpu()
    nan = torch.isnan(p_after)
    assert torch.equal(b.view("wc").cpu()[~nan], p_after.bfloat16().view(torch.int16)[~nan])
    assert torch.equal(torch.isnan(b.view("wc").cpu().view(torch.bfloat16)), nan)


# ------------------------------------------------------------------ frozen ranges
def _frozen_mask(n):
    """64-element-aligned frozen ranges at the start, in the middle and at the end, as ParamStore lays parameters out"""
    mask = np.ones(n, np.uint8)
    mask[:128] = 0
    mask[n // 128 * 64:n // 128 * 64 + 192] = 0
    mask[(n - 64) // 64 * 64:] = 0
    return mask


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_mask_freezes_p_m_v_wc_and_zero_grad_clears_everything(kind, zero_grad):
    n = 64 * 50
    h = _h(**dict(ADAM if kind == "adam" else SGD, step=4))
    before = _family(kind, n, 33, h)
    mask = _frozen_mask(n)
    frozen = mask == 0
    runs = {}
    for use_mask in (False, True):
        b = Bufs(n, mask=mask, **before)
        assert _launch(kind, b.desc(h, mask=use_mask, zero_grad=zero_grad)) == 0
        assert b.guards_intact()
        _check_step(kind, b, before, h, mask if use_mask else None)
        if zero_grad:
            assert not b.bits("g").any(), "g must be +0.0 everywhere, frozen ranges included"
        else:
            assert np.array_equal(b.bits("g"), _i32(before["g"]))
        runs[use_mask] = {k: b.bits(k) for k in ("p", "m", "v", "wc")}
    for k in ("p", "m", "v"):
        assert np.array_equal(runs[True][k][frozen], _i32(before[k])[frozen]), k            # recognisable: the family's values
        assert np.array_equal(runs[True][k][~frozen], runs[False][k][~frozen]), k
    assert np.all(runs[True]["wc"][frozen] == 0x1234)
    assert np.array_equal(runs[True]["wc"][~frozen], runs[False]["wc"][~frozen])
    assert (runs[False]["p"] != _i32(before["p"]))[frozen].any()                              # without the mask they do move


# ------------------------------------------------------------------ sub-range launches (side stream, DDP buckets)
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("n,cuts", [(64 * 50, (8, 1000, 2048)), (BIG, (BIG * 19 // 20 // 8 * 8,))])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_sub_range_launches_are_bit_identical_to_one_launch(kind, n, cuts, use_mask):
    """the pieces _FusedBase._launch makes: offsets are multiples of 8 (bucket boundaries, the engine's 95 % cut)"""
    h = _h(**dict(ADAM if kind == "adam" else SGD, step=6))
    before = _family(kind, n, 44, h)
    mask = _frozen_mask(n)
    whole = Bufs(n, mask=mask, **before)
    assert _launch(kind, whole.desc(h, mask=use_mask, zero_grad=1)) == 0
    parts = Bufs(n, mask=mask, **before)
    edges = (0,) + tuple(cuts) + (n,)
    assert all(c % 8 == 0 for c in cuts)
    for lo, hi in reversed(list(zip(edges, edges[1:]))):           # (the side stream's piece is the upper one and goes first)
        assert _launch(kind, parts.desc(h, mask=use_mask, zero_grad=1, off=lo, cnt=hi - lo)) == 0
    assert whole.guards_intact() and parts.guards_intact()
    for k in whole.full:
        assert torch.equal(whole.full[k].view(torch.uint8), parts.full[k].view(torch.uint8)), k
    assert not torch.equal(whole.view("p"), torch.from_numpy(before["p"]).cuda())


# ------------------------------------------------------------------ argument checks: DYK_ERR_ARG, nothing written
BAD = ["n_not_4", "n_zero", "n_negative", "step_zero", "step_negative", "p_misaligned", "g_misaligned", "m_misaligned",
       "v_misaligned", "wc_misaligned", "mask_misaligned", "p_null", "g_null", "m_null", "v_null"]


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bad_descriptors_are_rejected_and_write_nothing(kind, bad):
    """the checks of optim.hip run before the launch: the return code is DYK_ERR_ARG and no byte of any buffer, guard bands
    included, changes.  (NULL v is valid for SGD: there the call succeeds and v is not touched.)"""
    n = 256
    h = _h(**dict(ADAM if kind == "adam" else SGD, step=2))
    before = _family(kind, n, 55, h)
    b = Bufs(n, **before)
    d = b.desc(h, mask=True, zero_grad=1)
    if bad == "n_not_4":
        d.n = n - 2
    elif bad == "n_zero":
        d.n = 0
    elif bad == "n_negative":
        d.n = -n
    elif bad == "step_zero":
        d.step = 0
    elif bad == "step_negative":
        d.step = -3
    elif bad.endswith("_misaligned"):
        k = bad.split("_")[0]
        setattr(d, k, getattr(d, k) + {"wc": 4, "mask": 2}.get(k, 8))         # off 8 / 16 bytes, off 4 bytes; inside the buffer
        d.n = n - 8
    elif bad.endswith("_null"):
        setattr(d, bad.split("_")[0], None)
    snap = b.snapshot()
    rc = _launch(kind, d)
    if kind == "sgd" and bad == "v_null":
        assert rc == 0
        assert np.array_equal(b.bits("v", full=True), snap["v"])
        return
    assert rc == ERR_ARG
    now = b.snapshot()
    for k in snap:
        assert np.array_equal(now[k], snap[k]), k


# ------------------------------------------------------------------ twelve steps against torch.optim, with a yardstick
def _trajectory_inputs(seed, n=1 << 16, steps=12):
    """a different gradient every step, its magnitude redrawn over six decades; [0, 1024) gets an exactly zero gradient every step,
    [1024, 2048) starts at p = 0 with gradients ten decades down: after a few steps of history its denominator is eps alone"""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen) * 0.1
    p0[1024:2048] = 0
    gs = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=gen))
        g[:1024] = 0
        g[1024:2048] *= 1e-10
        gs.append(g)
    return p0, gs


def _torch_trajectory(make, p0, gs, dtype):
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = make([p])
    out = []
    for g in gs:
        p.grad = g.to(dtype).clone()
        opt.step()
        out.append(p.detach().double().clone())
    return out


def _kernel_trajectory(kind, h, p0, gs):
    n = p0.numel()
    z = np.zeros(n, np.float32)
    b = Bufs(n, p=p0.numpy(), g=z, m=z, v=z)
    out = []
    for t, g in enumerate(gs, 1):
        b.set(g=g.numpy())
        assert _launch(kind, b.desc(dict(h, step=t), zero_grad=1)) == 0
        out.append(b.view("p").cpu().double())
    assert b.guards_intact()
    return out


def _yardstick(kind, h, make):
    p0, gs = _trajectory_inputs(0)
    r64 = _torch_trajectory(make, p0, gs, torch.float64)
    r32 = _torch_trajectory(make, p0, gs, torch.float32)
    got = _kernel_trajectory(kind, h, p0, gs)
    lr = h["lr"]
    e_k = [float((a - r).abs().max()) / lr for a, r in zip(got, r64)]
    e_t = [float((a - r).abs().max()) / lr for a, r in zip(r32, r64)]
    print("%s E_k/lr: %s" % (kind, ["%.3e" % e for e in e_k]))
    print("%s E_t/lr: %s" % (kind, ["%.3e" % e for e in e_t]))
    print("%s E_k/E_t: %s" % (kind, ["%.2f" % (a / b) for a, b in zip(e_k, e_t)]))
    assert all(e > 0 for e in e_t)
    return e_k, e_t


def test_adam_trajectory_is_as_close_to_fp64_as_torch_fp32_is():
    """Twelve steps, real double-precision hyper-parameters on torch's side, fp32 ones in the descriptor.  E = max|p - p64| / lr
    after every step, for the kernel (E_k) and for torch.optim.Adam in fp32 on the CPU (E_t), both against torch.optim.Adam in
    fp64.  MEASURED on MI355X, E_k / E_t per step:
        1.00 at every one of the twelve steps (E_k = E_t to four digits, 6.4e-5 ... 1.06e-4)
    -- through step 7 both are set by ONE element whose first decayed gradient g + wd*p cancels to the size of eps (g = 1.6019e-5,
    wd*p = -1.6018e-5): the update is ill-conditioned there and the two fp32 evaluations round that sum alike.
    OPTIM_K['adam'] (tests/helpers.py) is twice the largest of them, rounded up to one digit, and may not exceed 4."""
    kw = dict(lr=1e-3, betas=(0.937, 0.999), eps=1e-8, weight_decay=5e-4)
    h = _h(lr=kw["lr"], beta1=kw["betas"][0], beta2=kw["betas"][1], eps=kw["eps"], weight_decay=kw["weight_decay"], grad_scale=1.0)
    e_k, e_t = _yardstick("adam", h, lambda ps: torch.optim.Adam(ps, foreach=False, **kw))
    assert OPTIM_K["adam"] <= 4
    for t, (a, b) in enumerate(zip(e_k, e_t), 1):
        assert a <= OPTIM_K["adam"] * b, (t, a, b)


def test_sgd_trajectory_is_as_close_to_fp64_as_torch_fp32_is():
    """The same for SGD-Nesterov (lr 1e-2, momentum 0.937, weight decay 5e-4).  MEASURED on MI355X, E_k / E_t per step:
        1.00 1.00 1.00 1.00 1.00 1.00 1.00 1.00 0.93 0.90 0.86 0.86      (E_k 1.5e-6 ... 1.1e-5)
    OPTIM_K['sgd'] is twice the largest of them, rounded up to one digit, and may not exceed 4."""
    kw = dict(lr=1e-2, momentum=0.937, weight_decay=5e-4, nesterov=True)
    h = _h(lr=kw["lr"], beta1=kw["momentum"], weight_decay=kw["weight_decay"], grad_scale=1.0)
    e_k, e_t = _yardstick("sgd", h, lambda ps: torch.optim.SGD(ps, foreach=False, **kw))
    assert OPTIM_K["sgd"] <= 4
    for t, (a, b) in enumerate(zip(e_k, e_t), 1):
        assert a <= OPTIM_K["sgd"] * b, (t, a, b)
