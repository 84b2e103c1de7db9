"""oracle/optim.py, the fp64 reference of the fused optimizer steps and its derived per-element bound (no GPU):
  * the reference is torch.optim.Adam / torch.optim.SGD(nesterov=True) in float64 up to the fp32 rounding of three scalars;
  * an fp32 evaluation in the statement order of the kernel's contract (include/dyk_hip.h, "Fused optimizer step": the
    torch.optim update rules with L2 weight decay added to the scaled gradient) stays at <= 0.5 of every bound;
  * the bound is not vacuous: each of six plausible mistakes exceeds it on at least half of the elements.
tests/test_gpu_optim.py holds the HIP kernels to the same reference and bound."""
import numpy as np
import pytest
import torch

from oracle.optim import adam_constants, adam_step_ref, input_family, sgd_step_ref

f32 = np.float32
STEPS = (1, 2, 10, 1000, 100000)
BETAS = ((0.937, 0.999), (0.5, 0.9))          # the project's, and an asymmetric pair
HYP = dict(lr=1e-3, eps=1e-8)


def _h32(**kw):
    """hyper-parameters as DykOptimDesc carries them: rounded to fp32, held in Python floats"""
    return {k: (float(f32(v)) if k != "step" else v) for k, v in kw.items()}


# ------------------------------------------------------------------ fp32 emulations (numpy float32, one rounding per operation)
def adam_emulation(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, grad_scale, step, kind=None):
    """fp32, statement by statement.  kind: None, or one deliberate mistake (swap / bc2 / epsin / adamw)"""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1 = f32(1.0 - float(b1) ** step)
    bc2 = 1.0 - float(b2) ** step
    bc2s = f32(bc2) if kind == "bc2" else f32(np.sqrt(bc2))
    ss = lr / bc1
    if kind == "swap":
        b1, b2 = b2, b1
    with np.errstate(all="ignore"):
        gr = g * gs
        if wd != 0 and kind != "adamw":
            gr = gr + wd * p
        m1 = b1 * m + (f32(1) - b1) * gr
        v1 = b2 * v + (f32(1) - b2) * gr * gr
        den = np.sqrt(v1 + eps) / bc2s if kind == "epsin" else np.sqrt(v1) / bc2s + eps
        p1 = p - ss * (m1 / den)
        if kind == "adamw":
            p1 = p1 - lr * wd * p
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def sgd_emulation(p, g, m, *, lr, beta1, weight_decay, grad_scale, step, kind=None):
    """kind: None, 'plain' (momentum without the Nesterov look-ahead), 'first' (the first-step rule m = g' at any step)"""
    lr, mom, wd, gs = (f32(x) for x in (lr, beta1, weight_decay, grad_scale))
    with np.errstate(all="ignore"):
        gr = g * gs
        if wd != 0:
            gr = gr + wd * p
        m1 = gr if (step == 1 or kind == "first") else mom * m + gr
        s = m1 if kind == "plain" else gr + mom * m1
        p1 = p - lr * s
    assert p1.dtype == m1.dtype == np.float32
    return p1, m1


def _ratio(got, ref, bound):
    """max |got - ref| / bound over all elements; 0/0 (exact results with a zero bound) counts as 0"""
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(err).all() and np.isfinite(bound).all()
    assert not ((bound == 0) & (err > 0)).any()
    return float(np.max(np.where(err > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


# ------------------------------------------------------------------ the reference is torch.optim in float64
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("step", [1, 2, 10, 1000])
@pytest.mark.parametrize("betas", BETAS)
def test_adam_reference_is_torch_adam_in_float64(betas, step, wd, grad_scale):
    """Same inputs = the fp32 values the descriptor carries, handed to torch as doubles.  What remains is the fp32 rounding of
    bc1, bc2_sqrt and step_size (three scalars, <= 3 x 2^-24 x (1 + ...) ~ 2e-7 relative on the update): 1e-6 relative on the
    update, plus the float64 rounding of p - update.  (With betas left in double the comparison would measure the rounding of
    beta2 instead: fl32(0.999) is 1.3e-5 of 1 - beta2 away from 0.999.  The trajectory tests of test_gpu_optim.py cover that
    with a yardstick.)"""
    h = _h32(lr=HYP["lr"], beta1=betas[0], beta2=betas[1], eps=HYP["eps"], weight_decay=wd, grad_scale=grad_scale, step=step)
    p, g, m, v = input_family(1 << 14, 3, "adam", h["beta1"], h["grad_scale"])
    p1, m1, v1 = adam_step_ref(p, g, m, v, **h)[:3]
    tp = torch.tensor(p, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"], foreach=False)
    tp.grad = torch.tensor(g, dtype=torch.float64) * h["grad_scale"]
    opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.tensor(m, dtype=torch.float64),
                         exp_avg_sq=torch.tensor(v, dtype=torch.float64))
    opt.step()
    P = p.astype(np.float64)
    d_t = tp.detach().numpy() - P
    assert np.abs(d_t).max() > 0
    assert np.all(np.abs((p1 - P) - d_t) <= 1e-6 * np.abs(d_t) + 2.0 ** -50 * np.abs(P))
    s = opt.state[tp]
    terms = np.abs(m) + np.abs(g) + np.abs(P)              # float64 rounding relative to the terms (the stripe cancels)
    assert np.all(np.abs(m1 - s["exp_avg"].numpy()) <= 1e-14 * terms)
    assert np.all(np.abs(v1 - s["exp_avg_sq"].numpy()) <= 1e-14 * (v + terms ** 2))


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("step", [1, 2, 10])
def test_sgd_reference_is_torch_sgd_nesterov_in_float64(step, wd, grad_scale):
    h = _h32(lr=1e-2, beta1=0.937, weight_decay=wd, grad_scale=grad_scale, step=step)
    p, g, m, _ = input_family(1 << 14, 4, "sgd", h["beta1"], h["grad_scale"])
    p1, m1 = sgd_step_ref(p, g, m, **h)[:2]
    tp = torch.tensor(p, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=h["lr"], momentum=h["beta1"], weight_decay=h["weight_decay"], nesterov=True, foreach=False)
    tp.grad = torch.tensor(g, dtype=torch.float64) * h["grad_scale"]
    if step > 1:
        opt.state[tp] = dict(momentum_buffer=torch.tensor(m, dtype=torch.float64))
    opt.step()
    P = p.astype(np.float64)
    d_t = tp.detach().numpy() - P
    assert np.abs(d_t).max() > 0
    assert np.all(np.abs((p1 - P) - d_t) <= 1e-6 * np.abs(d_t) + 2.0 ** -50 * np.abs(P))
    assert np.all(np.abs(m1 - opt.state[tp]["momentum_buffer"].numpy()) <= 1e-14 * (np.abs(m) + np.abs(g) + np.abs(P)))


def test_frozen_elements_pass_through_with_a_zero_bound():
    h = _h32(lr=1e-3, beta1=0.937, beta2=0.999, eps=1e-8, weight_decay=5e-4, grad_scale=1.0, step=3)
    p, g, m, v = input_family(256, 5)
    mask = np.ones(256, np.uint8)
    mask[64:128] = 0
    full, part = adam_step_ref(p, g, m, v, **h), adam_step_ref(p, g, m, v, mask, **h)
    live = mask.astype(bool)
    for a, b, old in zip(full[:3], part[:3], (p, m, v)):
        assert np.array_equal(a[live], b[live]) and np.array_equal(b[~live], old[~live].astype(np.float64))
    for b in part[3:]:
        assert np.all(b[~live] == 0) and np.all(b[live] > 0)
    sp = sgd_step_ref(p, g, m, v, mask, **h)
    assert np.array_equal(sp[0][~live], p[~live]) and np.array_equal(sp[2], v.astype(np.float64)) and np.all(sp[5] == 0)
    assert sgd_step_ref(p, g, m, None, **h)[2] is None


# ------------------------------------------------------------------ the bound holds for fp32 arithmetic, with headroom
@pytest.mark.parametrize("grad_scale", [1.0, 1 / 8, 1 / 65536])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("betas", BETAS)
def test_fp32_adam_emulation_has_twofold_headroom(betas, wd, grad_scale):
    worst = {}
    for step in STEPS:
        h = _h32(lr=HYP["lr"], beta1=betas[0], beta2=betas[1], eps=HYP["eps"], weight_decay=wd, grad_scale=grad_scale, step=step)
        p, g, m, v = input_family(1 << 20, 0, "adam", h["beta1"], h["grad_scale"])
        ref = adam_step_ref(p, g, m, v, **h)
        got = adam_emulation(p, g, m, v, **h)
        worst[step] = tuple(round(_ratio(a, r, b), 3) for a, r, b in zip(got, ref[:3], ref[3:]))
    print("adam emulation / bound (p, m, v) per step:", betas, wd, grad_scale, worst)
    assert max(max(w) for w in worst.values()) <= 0.5, worst


@pytest.mark.parametrize("grad_scale", [1.0, 1 / 8, 1 / 65536])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_fp32_sgd_emulation_has_twofold_headroom(wd, grad_scale):
    worst = {}
    for step in STEPS:
        h = _h32(lr=1e-2, beta1=0.937, weight_decay=wd, grad_scale=grad_scale, step=step)
        p, g, m, _ = input_family(1 << 20, 1, "sgd", h["beta1"], h["grad_scale"])
        ref = sgd_step_ref(p, g, m, **h)
        got = sgd_emulation(p, g, m, **h)
        worst[step] = (round(_ratio(got[0], ref[0], ref[3]), 3), round(_ratio(got[1], ref[1], ref[4]), 3))
    print("sgd emulation / bound (p, m) per step:", wd, grad_scale, worst)
    assert max(max(w) for w in worst.values()) <= 0.5, worst


def test_kernel_constants_follow_the_descriptor():
    omb1, omb2, bc1, bc2s, ss = adam_constants(0.937, 0.999, 1e-3, 1)
    b1, b2 = f32(0.937), f32(0.999)
    assert omb1 == float(f32(1) - b1) and omb2 == float(f32(1) - b2)
    assert bc1 == omb1 and bc2s == float(f32(np.sqrt(1.0 - float(b2))))          # step 1: bc = 1 - beta, exactly
    assert ss == float(f32(1e-3) / f32(bc1))
    assert adam_constants(0.937, 0.999, 1e-3, 100000)[2:4] == (1.0, 1.0)


# ------------------------------------------------------------------ the bound is not vacuous
@pytest.mark.parametrize("step", [1, 10, 1000, 100000])
def test_adam_bound_catches_the_usual_mistakes(step):
    """share of the elements of p beyond the bound: 0 for the emulation, at least one half for each mistake.  At step 100000
    sqrt(bc2) and bc2 are both 1 in fp32, so that mistake cannot be seen there by construction and is left out."""
    h = _h32(lr=1e-3, beta1=0.937, beta2=0.999, eps=1e-8, weight_decay=5e-4, grad_scale=0.5, step=step)
    p, g, m, v = input_family(1 << 20, 0, "adam", h["beta1"], h["grad_scale"])
    ref = adam_step_ref(p, g, m, v, **h)
    share = {}
    for kind in (None, "swap", "bc2", "epsin", "adamw"):
        p1 = adam_emulation(p, g, m, v, kind=kind, **h)[0]
        share[kind] = float(np.mean(np.abs(p1.astype(np.float64) - ref[0]) > ref[3]))
    print("adam step %d: share of elements beyond bound_p:" % step, share)
    assert share.pop(None) == 0.0
    if step == 100000:
        share.pop("bc2")
    assert min(share.values()) >= 0.5, share


@pytest.mark.parametrize("step", [2, 10, 1000])
def test_sgd_bound_catches_the_usual_mistakes(step):
    """plain instead of Nesterov momentum, and the first-step rule (m = g') used after the first step: both change the update
    by a term of the size of momentum * m"""
    h = _h32(lr=1e-2, beta1=0.937, weight_decay=5e-4, grad_scale=0.5, step=step)
    p, g, m, _ = input_family(1 << 20, 1, "sgd", h["beta1"], h["grad_scale"])
    ref = sgd_step_ref(p, g, m, **h)
    share = {}
    for kind in (None, "plain", "first"):
        p1, m1 = sgd_emulation(p, g, m, kind=kind, **h)
        share[kind] = (float(np.mean(np.abs(p1.astype(np.float64) - ref[0]) > ref[3])),
                       float(np.mean(np.abs(m1.astype(np.float64) - ref[1]) > ref[4])))
    print("sgd step %d: share of elements beyond (bound_p, bound_m):" % step, share)
    assert share.pop(None) == (0.0, 0.0)
    assert min(s[0] for s in share.values()) >= 0.5, share
    assert share["first"][1] >= 0.5


def test_sgd_first_step_ignores_the_momentum_buffer():
    h = _h32(lr=1e-2, beta1=0.937, weight_decay=5e-4, grad_scale=1.0, step=1)
    p, g, m, _ = input_family(1 << 12, 2, "sgd")
    a, b = sgd_step_ref(p, g, m, **h), sgd_step_ref(p, g, np.full_like(m, np.nan), **h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------ the argument checks come before the launch
def _fake_desc(n=64, step=1):
    from dyk import lib
    d = lib.DykOptimDesc()
    d.p, d.g, d.m, d.v, d.wc, d.mask = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    d.n, d.step, d.zero_grad = n, step, 1
    d.lr, d.beta1, d.beta2, d.eps, d.weight_decay, d.grad_scale = 1e-3, 0.937, 0.999, 1e-8, 5e-4, 1.0
    return d


BAD = ["null", "n_not_4", "n_zero", "n_negative", "step_zero", "step_negative", "p_misaligned", "g_misaligned", "m_misaligned",
       "v_misaligned", "wc_misaligned", "mask_misaligned", "p_null", "g_null", "m_null", "v_null"]


@pytest.mark.parametrize("fn,bad", [(fn, bad) for fn in ("dyk_adam_step", "dyk_sgd_step") for bad in BAD
                                    if (fn, bad) != ("dyk_sgd_step", "v_null")])          # NULL v is valid for SGD
def test_bad_optimizer_descriptors_are_rejected_before_any_launch(fn, bad):
    """no GPU here: a launch would fail with DYK_ERR_HIP, not DYK_ERR_ARG (-1).  The addresses are never dereferenced.
    (tests/test_gpu_optim.py repeats this on the device and checks that no buffer changes.)"""
    import ctypes
    from dyk import lib
    call = getattr(lib.load(), fn)
    if bad == "null":
        assert call(None, None) == -1
        return
    d = _fake_desc()
    if bad == "n_not_4":
        d.n = 62
    elif bad == "n_zero":
        d.n = 0
    elif bad == "n_negative":
        d.n = -64
    elif bad == "step_zero":
        d.step = 0
    elif bad == "step_negative":
        d.step = -1
    elif bad.endswith("_misaligned"):
        k = bad.split("_")[0]
        setattr(d, k, getattr(d, k) + {"wc": 4, "mask": 2}.get(k, 8))
    else:
        setattr(d, bad.split("_")[0], None)
    assert call(ctypes.byref(d), None) == -1
