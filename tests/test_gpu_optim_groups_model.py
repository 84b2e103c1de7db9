"""Parameter groups and decoupled weight decay through the public classes: FusedAdam / FusedSGD(param_groups=...), FusedAdamW,
dyk.optim.yolo_param_groups, per-group LR schedules, checkpoints exchanged with torch.optim.AdamW, the guarded grouped step and
frozen parameters.  Smallest cfg and image size of the model tests (tests/test_gpu_harness.py)."""
import io

import numpy as np
import pytest
import torch

import optim_groups_ref as R
from helpers import C1, OPTIM_K
from test_gpu_harness import _backward, _batch, _bf16_packs, _model

pytestmark = pytest.mark.gpu

BETAS = (0.937, 0.999)
WD = 5e-4


def _bits(t):
    return t.detach().view(torch.int32).cpu().clone()


def _kinds(m, groups):
    """entry name -> index of its group (None: in no group)"""
    of = {id(p): k for k, g in enumerate(groups) for p in g["params"]}
    return {e.name: of.get(id(e.param)) for e in m.engine.store.entries}


# ------------------------------------------------------------------ three steps against torch.optim over the same groups
def _torch_steps(make, P0, grads, gmap, hypers, dtype):
    """torch.optim over one tensor per group (the elements of that group, gathered: the update is elementwise) -> the flat
    parameters after every step, float64"""
    idx = [torch.nonzero(gmap == k + 1).flatten() for k in range(len(hypers))]
    ps = [P0[i].to(dtype).clone().requires_grad_(True) for i in idx]
    opt = make([dict(h, params=[p]) for h, p in zip(hypers, ps)])
    out = []
    for G in grads:
        for p, i in zip(ps, idx):
            p.grad = G[i].to(dtype).clone()
        opt.step()
        flat = P0.double().clone()
        for p, i in zip(ps, idx):
            flat[i] = p.detach().double()
        out.append(flat)
    return out


@pytest.mark.parametrize("which", ["adam_yolo_groups", "adamw"])
def test_three_step_trajectory_is_as_close_to_fp64_as_torch_fp32_is(which):
    """three steps with a different gradient each (G scaled by a per-element factor in [-2, 2] before steps 2 and 3, as
    tests/test_gpu_model.py varies it); after every step the fused result may be at most OPTIM_K times as far from torch.optim in
    fp64 as torch.optim in fp32 is -- both torch runs over the same parameter groups"""
    from dyk.optim import FusedAdam, FusedAdamW, yolo_param_groups
    m = _model(C1)
    _backward(m, _batch(70))
    st = m.engine.store
    P0, G0 = st.P.clone(), st.G.clone()
    if which == "adam_yolo_groups":
        groups = yolo_param_groups(m, WD, bias_lr=2e-3)
        fused = FusedAdam(m, lr=1e-3, betas=BETAS, param_groups=groups)
        hypers = [dict(weight_decay=WD), dict(weight_decay=0.0), dict(weight_decay=0.0, lr=2e-3)]
        make = lambda gs: torch.optim.Adam(gs, lr=1e-3, betas=BETAS, foreach=False)
    else:
        fused = FusedAdamW(m, lr=1e-3, betas=BETAS)
        assert fused.param_groups[0]["weight_decay"] == 1e-2
        hypers = [dict()]
        make = lambda gs: torch.optim.AdamW(gs, lr=1e-3, betas=BETAS, foreach=False)
    fused.zero_in_step = False
    gen = torch.Generator().manual_seed(5)
    grads = [G0]
    for _ in range(2):
        grads.append(grads[-1] * (torch.rand(G0.numel(), generator=gen) * 4 - 2).cuda())
    got = []
    for G in grads:
        with torch.no_grad():
            st.G.copy_(G)
        fused.step()
        got.append(st.P.detach().double().clone())
    gmap = fused._gmap
    assert gmap is not None and int(gmap.max()) == len(hypers)
    r32 = _torch_steps(make, P0, grads, gmap, hypers, torch.float32)
    r64 = _torch_steps(make, P0, grads, gmap, hypers, torch.float64)
    assert not torch.equal(got[2], got[1])
    for t in range(3):
        e_k, e_t = float((got[t] - r64[t]).abs().max()), float((r32[t] - r64[t]).abs().max())
        print("%s step %d: E_k %.3e E_t %.3e ratio %.2f" % (which, t + 1, e_k, e_t, e_k / e_t))
        assert e_t > 0 and e_k <= OPTIM_K["adam"] * e_t, (which, t, e_k, e_t)


# ------------------------------------------------------------------ weight decay reaches the decay group only
def test_weight_decay_reaches_only_the_decay_group():
    """zero gradients, one FusedSGD step: p' = p - lr * (1 + momentum) * wd * p where decay applies, p' = p - lr * 0 elsewhere.
    With yolo_param_groups BatchNorm scales / shifts and biases keep their bits; with ONE group the same tensors move."""
    from dyk.optim import FusedSGD, yolo_param_groups
    moved = {}
    for grouped in (True, False):
        m = _model(C1)
        _backward(m, _batch(71))
        st = m.engine.store
        groups = yolo_param_groups(m, WD)
        kinds = _kinds(m, groups)
        if grouped:
            opt = FusedSGD(m, lr=1e-2, momentum=0.937, param_groups=groups)
        else:
            opt = FusedSGD(m, lr=1e-2, momentum=0.937, weight_decay=WD)
        assert opt._grouped() == grouped
        with torch.no_grad():
            st.G.zero_()
        before = _bits(st.P)
        opt.step()
        after = _bits(st.P)
        moved[grouped] = {e.name: not torch.equal(before[e.offset:e.offset + e.numel], after[e.offset:e.offset + e.numel])
                          for e in st.entries if bool(st.P[e.offset:e.offset + e.numel].any())}
    assert set(kinds.values()) == {0, 1, 2}
    decay = [n for n in moved[True] if kinds[n] == 0]
    rest = [n for n in moved[True] if kinds[n] != 0]
    assert len(decay) > 50 and len(rest) > 100
    assert all(moved[True][n] for n in decay)
    assert not any(moved[True][n] for n in rest), [n for n in rest if moved[True][n]][:5]
    assert all(moved[False][n] for n in decay) and all(moved[False][n] for n in rest)


# ------------------------------------------------------------------ per-group schedules
def test_lambda_lr_with_a_lambda_per_group_equals_hand_set_learning_rates():
    from dyk.optim import FusedAdam, yolo_param_groups
    lambdas = [lambda e: 1.0 / (1 + e), lambda e: 0.5 ** e, lambda e: 2.0 - 0.75 * e]
    batches = [_batch(72 + i) for i in range(3)]
    out = []
    for scheduled in (True, False):
        m = _model(C1)
        opt = FusedAdam(m, lr=1e-3, betas=BETAS, param_groups=yolo_param_groups(m, WD, bias_lr=3e-3))
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambdas) if scheduled else None
        for e, b in enumerate(batches):
            if not scheduled:
                for g, base, lam in zip(opt.param_groups, (1e-3, 1e-3, 3e-3), lambdas):
                    g["lr"] = base * lam(e)
            _backward(m, b)
            opt.step()
            if scheduled:
                sched.step()
        out.append((_bits(m.engine.store.P), [g["lr"] for g in opt.param_groups]))
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1] == [1e-3 * lambdas[0](3), 1e-3 * lambdas[1](3), 3e-3 * lambdas[2](3)]
    # ... and the rates did matter: the same three steps at constant rates end elsewhere
    m = _model(C1)
    opt = FusedAdam(m, lr=1e-3, betas=BETAS, param_groups=yolo_param_groups(m, WD, bias_lr=3e-3))
    for b in batches:
        _backward(m, b)
        opt.step()
    assert not torch.equal(_bits(m.engine.store.P), out[0][0])


# ------------------------------------------------------------------ checkpoints in torch.optim's multi-group format
def test_checkpoint_goes_through_torch_adamw_and_back_and_resumes_bit_for_bit():
    from dyk.optim import FusedAdamW, yolo_param_groups
    b = [_batch(80 + i) for i in range(3)]
    m = _model(C1)
    opt = FusedAdamW(m, lr=1e-3, betas=BETAS, param_groups=yolo_param_groups(m, 1e-2, bias_lr=2e-3))
    for i in range(2):
        _backward(m, b[i])
        opt.step()
    osd = opt.state_dict()
    assert [len(g["params"]) for g in osd["param_groups"]] == [len(g["params"]) for g in opt.param_groups] and len(osd["param_groups"]) == 3
    assert [g["weight_decay"] for g in osd["param_groups"]] == [1e-2, 0.0, 0.0] and osd["param_groups"][2]["lr"] == 2e-3
    assert all(g["decoupled_weight_decay"] is True for g in osd["param_groups"])
    n_params = sum(len(g["params"]) for g in opt.param_groups)
    assert sorted(osd["state"]) == list(range(n_params)) and float(osd["state"][n_params - 1]["step"]) == 2.0
    buf = io.BytesIO()
    torch.save({"model": m.state_dict(), "optimizer": osd}, buf)
    _backward(m, b[2])
    opt.step()
    want = _bits(m.engine.store.P)
    # fused -> torch.optim.AdamW over the same groups of a second model
    buf.seek(0)
    ck = torch.load(buf)
    m2 = _model(C1)
    m2.load_state_dict(ck["model"])
    m2.train()
    if m2.engine.store.P is None:
        with torch.no_grad():
            m2.engine.store.adopt(torch.device("cuda", 0))
    groups2 = yolo_param_groups(m2, 1e-2, bias_lr=2e-3)
    topt = torch.optim.AdamW(groups2, lr=1e-3, betas=BETAS)
    topt.load_state_dict(ck["optimizer"])
    assert [g["weight_decay"] for g in topt.param_groups] == [1e-2, 0.0, 0.0] and topt.param_groups[2]["lr"] == 2e-3
    p_last = groups2[2]["params"][-1]
    assert float(topt.state[p_last]["step"]) == 2.0 and topt.state[p_last]["exp_avg"].shape == p_last.shape
    # ... and back: torch's state_dict into a fresh fused optimizer, which continues like the uninterrupted run
    back = topt.state_dict()
    opt2 = FusedAdamW(m2, lr=1e-3, betas=BETAS, param_groups=yolo_param_groups(m2, 1e-2, bias_lr=2e-3))
    opt2.load_state_dict(back)
    assert opt2._t == 2 and opt2._grouped() and [g["lr"] for g in opt2.param_groups] == [1e-3, 1e-3, 2e-3]
    _backward(m2, b[2])
    opt2.step()
    assert torch.equal(_bits(m2.engine.store.P), want)


# ------------------------------------------------------------------ the guarded grouped step
def test_guarded_grouped_step_clips_skips_and_counts():
    from dyk.optim import FusedAdam, yolo_param_groups
    m = _model(C1)
    _backward(m, _batch(90))
    st = m.engine.store
    g0, p0 = st.G.cpu().numpy().copy(), st.P.cpu().numpy().copy()
    ref_norm = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    groups = yolo_param_groups(m, WD, bias_lr=2e-3)
    opt = FusedAdam(m, lr=1e-3, betas=BETAS, param_groups=groups, max_grad_norm=0.5 * ref_norm, skip_nonfinite=True)
    opt.step()                                                   # clipped
    s = opt.grad_stats(wait=True)
    assert abs(s["norm"] - ref_norm) <= 2.0 ** -23 * ref_norm and 0.49 < s["clip_coef"] < 0.51
    assert s["applied_steps"] == 1 and s["skipped_steps"] == 0 and s["nonfinite"] == 0
    gmap = opt._gmap.cpu().numpy()
    z = np.zeros_like(p0)
    hyp = [dict(lr=1e-3, weight_decay=WD), dict(lr=1e-3, weight_decay=0.0), dict(lr=2e-3, weight_decay=0.0)]
    ref = R.grouped_step_ref("adam", p0, g0, z, z, gmap, hyp, beta1=float(np.float32(BETAS[0])), beta2=float(np.float32(BETAS[1])),
                             eps=float(np.float32(1e-8)), grad_scale=float(np.float32(s["clip_coef"])), step=1)
    got = st.P.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref[0]) <= ref[3]) and np.abs(got - p0).max() > 0
    assert not bool(st.G.any())
    p1, m1, v1 = _bits(st.P), _bits(opt._m), _bits(opt._v)
    _backward(m, _batch(91))
    victim = groups[2]["params"][0]                             # a bias: the smallest group decides for all of them
    victim.grad.view(-1)[0] = float("inf")
    opt.step()                                                   # skipped
    s = opt.grad_stats(wait=True)
    assert s["applied_steps"] == 1 and s["skipped_steps"] == 1 and s["nonfinite"] == 1
    assert torch.equal(_bits(st.P), p1) and torch.equal(_bits(opt._m), m1) and torch.equal(_bits(opt._v), v1)
    assert not bool(st.G.any()), "the skipped step clears the gradients as an applied one does"
    _backward(m, _batch(92))
    opt.step()
    s = opt.grad_stats(wait=True)
    assert s["applied_steps"] == 2 and s["skipped_steps"] == 1 and not torch.equal(_bits(st.P), p1)
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0


# ------------------------------------------------------------------ frozen parameters
def test_frozen_prefix_with_groups_keeps_its_bits_and_gets_no_grad():
    from dyk.optim import FusedAdamW, yolo_param_groups
    m = _model(C1)
    frozen = [p for idx in range(10) for p in m.module_list[idx].parameters()]
    for p in frozen:
        p.requires_grad_(False)
    groups = yolo_param_groups(m, 1e-2)
    assert not {id(p) for p in frozen} & {id(p) for g in groups for p in g["params"]}
    opt = FusedAdamW(m, lr=1e-3, betas=BETAS, param_groups=groups)
    _backward(m, _batch(93))
    st = m.engine.store
    before = _bits(st.P)
    opt.step()
    after = _bits(st.P)
    gmap = opt._gmap.cpu()
    n_frozen = n_live = 0
    for e in st.entries:
        sl = slice(e.offset, e.offset + e.numel)
        if e.param.requires_grad:
            n_live += int(not torch.equal(before[sl], after[sl]))
            assert bool((gmap[sl] > 0).all())
        else:
            n_frozen += 1
            assert e.param.grad is None and torch.equal(before[sl], after[sl]), e.name
            assert not bool(gmap[sl].any()) and not bool(opt._m[sl].any()) and not bool(opt._v[sl].any())
    assert n_frozen == len(frozen) > 0 and n_live > 100


def test_bf16_copy_after_a_grouped_step_with_an_overwritten_frozen_tensor_equals_a_rebuild(tiles):
    """grouped mode always has a mask, so the frozen-overwritten rule of dyk.optim._FusedBase._desc applies: the bf16 copy the
    kernel writes is complete only if it was current when the step began (tests/test_gpu_harness.py, `frozen_overwritten`)"""
    from dyk.optim import FusedAdam, yolo_param_groups
    assert tiles == "pinned"
    m = _model(C1, "bf16")
    for idx in range(10):
        for p in m.module_list[idx].parameters():
            p.requires_grad_(False)
    opt = FusedAdam(m, lr=1e-3, betas=BETAS, param_groups=yolo_param_groups(m, WD))
    _backward(m, _batch(94))
    st = m.engine.store
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for e in st.entries:
        if not e.param.requires_grad:
            sd[e.name] = sd[e.name] * 1.25 + 0.01
    m.load_state_dict(sd)
    opt.step()
    torch.cuda.synchronize()
    got = _bf16_packs(st)
    st.compute_weights(torch.bfloat16, force=True)
    torch.cuda.synchronize()
    want = _bf16_packs(st)
    stale = [k for k in got if not torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8))]
    assert not stale, "bf16 staging buffers differ from a rebuild from P: %s" % stale
    assert torch.equal(want["Wc"].view(torch.int16), st.P.bfloat16().view(torch.int16))
