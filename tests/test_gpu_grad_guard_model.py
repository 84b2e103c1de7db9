"""The gradient guard through the public classes: FusedAdam(max_grad_norm=, skip_nonfinite=), grad_stats(), checkpoints of a run
with a skipped step, dyk.optim.clip_grad_norm_ with a stock torch.optim on the gradient views, frozen parameters -- and the
default path, which must stay what it was.  Smallest cfg and image size of the model tests (tests/test_gpu_harness.py)."""
import io

import numpy as np
import pytest
import torch

from helpers import C1
from oracle.optim import adam_step_ref
from test_gpu_harness import _backward, _batch, _model

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)


def _bits(t):
    return t.detach().view(torch.int32).cpu().clone()


def test_default_path_allocates_no_record_and_is_reproducible():
    from dyk.optim import FusedAdam
    out = []
    for _ in range(2):
        m = _model(C1)
        opt = FusedAdam(m, **KW)
        for i in range(2):
            _backward(m, _batch(20 + i))
            opt.step()
        assert opt._rec is None and opt._stats_ws is None and not opt._guarded and opt.grad_stats(wait=True) is None
        assert opt._t == 2
        out.append(_bits(m.engine.store.P))
    assert torch.equal(out[0], out[1])


def test_skip_nonfinite_skips_the_poisoned_step_and_checkpoints_the_applied_count():
    from dyk.optim import FusedAdam
    b = [_batch(30 + i) for i in range(4)]
    m = _model(C1)
    opt = FusedAdam(m, skip_nonfinite=True, **KW)
    st = m.engine.store
    _backward(m, b[0])
    opt.step()                                                   # clean
    s = opt.grad_stats(wait=True)
    assert s["applied_steps"] == 1 and s["skipped_steps"] == 0 and s["nonfinite"] == 0 and s["clip_coef"] == 1.0
    assert np.isfinite(s["norm"]) and s["norm"] > 0
    p1 = _bits(st.P)
    m1, v1 = _bits(opt._m), _bits(opt._v)
    _backward(m, b[1])
    victim = [p for p in m.parameters() if p.requires_grad][3]
    victim.grad[(0,) * victim.grad.dim()] = float("inf")         # one element of one trainable gradient view
    opt.step()                                                   # poisoned: skipped on the device
    assert torch.equal(_bits(st.P), p1) and torch.equal(_bits(opt._m), m1) and torch.equal(_bits(opt._v), v1)
    assert not bool(st.G.any()), "the skipped step clears the gradients as an applied one does"
    s = opt.grad_stats(wait=True)
    assert s["applied_steps"] == 1 and s["skipped_steps"] == 1 and s["nonfinite"] == 1
    _backward(m, b[2])
    opt.step()                                                   # clean
    s = opt.grad_stats(wait=True)
    assert s["skipped_steps"] == 1 and s["applied_steps"] == 2 and s["nonfinite"] == 0
    assert not torch.equal(_bits(st.P), p1)
    osd = opt.state_dict()
    assert float(osd["state"][0]["step"]) == 2.0
    buf = io.BytesIO()
    torch.save({"model": m.state_dict(), "optimizer": osd}, buf)
    _backward(m, b[3])
    opt.step()
    want = _bits(st.P)
    assert opt.grad_stats(wait=True)["applied_steps"] == 3
    # a new optimizer loaded from the checkpoint continues bit for bit (Adam's t = 3 for its first step, not 4)
    buf.seek(0)
    ck = torch.load(buf)
    m2 = _model(C1)
    m2.load_state_dict(ck["model"])
    m2.train()
    opt2 = FusedAdam(m2, skip_nonfinite=True, **KW)
    if m2.engine.store.P is None:
        with torch.no_grad():
            m2.engine.store.adopt(torch.device("cuda", 0))
    opt2.load_state_dict(ck["optimizer"])
    _backward(m2, b[3])
    opt2.step()
    assert torch.equal(_bits(m2.engine.store.P), want)
    s2 = opt2.grad_stats(wait=True)
    assert s2["applied_steps"] == 3 and s2["skipped_steps"] == 0
    assert float(opt2.state_dict()["state"][0]["step"]) == 3.0


def test_max_grad_norm_equals_an_unguarded_step_with_the_reported_coefficient():
    from dyk.optim import FusedAdam
    batch = _batch(40)
    probe = _model(C1)
    _backward(probe, batch)
    po = FusedAdam(probe, skip_nonfinite=True, **KW)
    g0 = probe.engine.store.G.cpu().numpy().copy()
    p0 = probe.engine.store.P.cpu().numpy().copy()
    po.step()
    norm = po.grad_stats(wait=True)["norm"]
    ref_norm = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    assert abs(norm - ref_norm) <= 2.0 ** -23 * ref_norm
    a = _model(C1)
    _backward(a, batch)
    assert torch.equal(a.engine.store.G.cpu(), torch.from_numpy(g0))
    oa = FusedAdam(a, max_grad_norm=0.5 * norm, **KW)
    oa.step()
    s = oa.grad_stats(wait=True)
    coef = s["clip_coef"]
    assert 0.49 < coef < 0.51 and s["norm"] == norm and s["applied_steps"] == 1
    b = _model(C1)
    _backward(b, batch)
    ob = FusedAdam(b, **KW)
    ob.grad_scale = coef
    ob.step()
    z = np.zeros_like(p0)
    ref = adam_step_ref(p0, g0, z, z, None, lr=KW["lr"], beta1=KW["betas"][0], beta2=KW["betas"][1], eps=1e-8,
                        weight_decay=KW["weight_decay"], grad_scale=coef, step=1)
    pa, pb = a.engine.store.P.cpu().numpy().astype(np.float64), b.engine.store.P.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(pa - ref[0]) <= ref[3]) and np.all(np.abs(pb - ref[0]) <= ref[3])
    assert np.all(np.abs(pa - pb) <= ref[3])
    assert np.abs(pa - p0).max() > 0


def test_clip_grad_norm_with_a_stock_optimizer_on_the_views():
    from dyk.optim import clip_grad_norm_
    m = _model(C1)
    sgd = torch.optim.SGD([p for p in m.parameters()], lr=1e-2)
    _backward(m, _batch(50))
    st = m.engine.store
    g0 = st.G.cpu().numpy().copy()
    p0 = _bits(st.P)
    ref = float(np.sqrt(np.sum(g0.astype(np.float64) ** 2)))
    norm = clip_grad_norm_(m, 0.5 * ref)
    assert isinstance(norm, torch.Tensor) and norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float32
    sgd.step()
    norm = float(norm)
    assert abs(norm - ref) <= 2.0 ** -23 * ref
    f = np.float32
    coef = f(0.5 * ref) / (f(norm) + f(1e-6))
    assert 0.49 < coef < 0.51
    assert np.array_equal(st.G.cpu().numpy().view(np.uint32), (g0 * coef).view(np.uint32))
    for p in list(m.parameters())[:5]:
        assert p.grad.data_ptr() >= st.G.data_ptr() and p.grad.data_ptr() < st.G.data_ptr() + 4 * st.total   # still the views
    assert not torch.equal(_bits(st.P), p0)
    # within the limit: nothing is scaled, the same norm comes back
    g1 = st.G.clone()
    again = clip_grad_norm_(m, 4 * ref)
    assert torch.equal(st.G, g1) and abs(float(again) - float(coef) * norm) <= 1e-6 * ref


def test_an_inf_in_the_frozen_range_of_G_does_not_cause_a_skip():
    from dyk.optim import FusedAdam
    m = _model(C1)
    frozen = []
    for idx in range(10):
        for p in m.module_list[idx].parameters():
            p.requires_grad_(False)
            frozen.append(p)
    assert frozen
    opt = FusedAdam(m, skip_nonfinite=True, max_grad_norm=1e9, **KW)
    _backward(m, _batch(60))
    st = m.engine.store
    e = next(e for e in st.entries if not e.param.requires_grad)
    live = next(e for e in st.entries if e.param.requires_grad)
    st.G[e.offset] = float("inf")
    st.G[e.offset + e.numel - 1] = float("nan")
    p0 = _bits(st.P)
    opt.step()
    s = opt.grad_stats(wait=True)
    assert s["skipped_steps"] == 0 and s["applied_steps"] == 1 and s["nonfinite"] == 0 and np.isfinite(s["norm"])
    p1 = _bits(st.P)
    assert torch.equal(p1[e.offset:e.offset + e.numel], p0[e.offset:e.offset + e.numel])
    assert not torch.equal(p1[live.offset:live.offset + live.numel], p0[live.offset:live.offset + live.numel])
    # the same values in a trainable range do
    _backward(m, _batch(61))
    st.G[live.offset] = float("inf")
    opt.step()
    s = opt.grad_stats(wait=True)
    assert s["skipped_steps"] == 1 and s["applied_steps"] == 1 and s["nonfinite"] == 1
    assert torch.equal(_bits(st.P), p1)
