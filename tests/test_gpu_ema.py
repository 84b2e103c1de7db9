"""ModelEMA on the GPU: the one-launch update (dyk_ema_update) is bit-identical to the reference's per-entry torch loop
(reference build_utils/torch_utils.py:108-120), the EMA model evaluates with the averaged weights, it does not disturb
training, deepcopy gives an independent model at any point of the original's life, and an EMA restored from a checkpoint
continues bit for bit.  Small cfg and shapes of test_gpu_model.py; tile choice pinned (fixture `tiles`) wherever two plans are
compared bit for bit."""
import copy
import io
import math

import pytest
import torch

from helpers import C2, hyp, oracle_net

pytestmark = pytest.mark.gpu


def _decay(x):
    return 0.9999 * (1 - math.exp(-x / 2000))


def _inputs():
    g = torch.Generator().manual_seed(1234)
    return torch.rand(2, 3, 128, 160, generator=g).cuda(), torch.rand(2, 3, 128, 160, generator=g).cuda()


def _model(dtype="fp32"):
    from build_utils.parse_config import materialize_cfg
    from models import YOLO
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(C2))
    m.load_state_dict(oracle_net(C2).synth_state(0))
    m.dyk_dtype = dtype
    m.nc, m.hyp, m.gr = 1, hyp(), 1.0
    return m.cuda()


TARGETS = torch.tensor([[0, 0, 0.30, 0.40, 0.20, 0.45], [0, 0, 0.70, 0.55, 0.12, 0.30], [1, 0, 0.50, 0.50, 0.25, 0.60]])


def _train_step(m, opt, x, y):
    """one step of the reference's loop: forward, compute_loss, backward, optimizer"""
    from build_utils.utils import compute_loss
    ld = compute_loss(m(x, y), TARGETS.cuda(), m)
    loss = ld["box_loss"] + ld["obj_loss"] + ld["class_loss"]
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach().clone()


def _heads(m, x, y):
    with torch.no_grad():
        _, p = m(x, y)
    return [t.detach().contiguous().clone() for t in p]


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _reference_update(esd, msd, d):
    """the reference's ModelEMA.update body (torch_utils.py:116-120) on state_dict snapshots"""
    for k, v in esd.items():
        if v.dtype.is_floating_point:
            v *= d
            v += (1. - d) * msd[k].detach()


def _snapshot(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _specials(n, g, phase):
    """n floats: normals over many magnitudes, and at every 7th element (from `phase`) a denormal, +-Inf or a NaN"""
    v = torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-30, 30, (n,), generator=g).float())
    bits = v.view(torch.int32)
    pick = torch.arange(phase, n, 7)
    special = torch.tensor([0x00000001, 0x007fffff, 0x80012345 - 2 ** 32, 0x7f800000, 0xff800000 - 2 ** 32, 0x7fc00000,
                            0xffc00000 - 2 ** 32, 0x7fa00001, 0x00400000], dtype=torch.int32)
    bits[pick] = special[torch.randint(0, len(special), (len(pick),), generator=g)]
    return v


@pytest.mark.parametrize("d", [0.0, 1e-9, 0.5, _decay(1), _decay(10 ** 6)])
def test_kernel_matches_torch_bitwise(d):
    from dyk.ema import launch
    g = torch.Generator().manual_seed(11)
    seen = torch.zeros(2, dtype=torch.bool)
    # two regions per launch: tiny, a partial last block (256 threads x 4 elements), and a grid-stride tail past 8192 blocks
    for sizes in [(4, 64), (64, 5 * 1024 + 12), (8192 * 1024 + 1028, 4)]:
        srcs = [_specials(n, g, 4).cuda() for n in sizes]                 # specials of src and dst at different elements:
        dsts = [_specials(n, g, 1).cuda() for n in sizes]                 # which NaN wins an add of two NaNs is not pinned
        refs = [t.clone() for t in dsts]
        for v, mv in zip(refs, srcs):
            v *= d
            v += (1. - d) * mv
        launch(list(zip(srcs, dsts)), d)
        torch.cuda.synchronize()
        for a, b in zip(dsts, refs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (d, sizes)
            seen |= torch.tensor([bool(torch.isnan(a).any()), bool(torch.isinf(a).any())])
    assert bool(seen.all())


@pytest.mark.parametrize("optimizer", ["fused", "torch_frozen_prefix"])
def test_model_ema_matches_the_reference_algorithm_bitwise(optimizer, tiles):
    from build_utils.torch_utils import ModelEMA
    from dyk.optim import FusedAdam
    m = _model().train()
    params = list(m.parameters())
    if optimizer == "fused":
        opt = FusedAdam(m, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    else:
        for p in params[:len(params) // 3]:
            p.requires_grad_(False)
        opt = torch.optim.Adam([p for p in params if p.requires_grad], lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    ema = ModelEMA(m)
    ref = _snapshot(ema.ema)
    nbt0 = {k: v.clone() for k, v in ref.items() if not v.dtype.is_floating_point}
    x, y = _inputs()
    for i in range(3):
        _train_step(m, opt, x, y)
        ema.update(m)
        _reference_update(ref, _snapshot(m), ema.decay(i + 1))
    assert ema.updates == 3
    got = ema.ema.state_dict()
    assert list(got) == list(ref)
    moved = 0
    for k, v in got.items():
        if v.dtype.is_floating_point:
            assert torch.equal(v.view(torch.int32), ref[k].view(torch.int32)), k
            moved += int(not torch.equal(v, m.state_dict()[k]))
        else:
            assert torch.equal(v, nbt0[k]), k
    assert moved > 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ema_model_evaluates_with_the_averaged_weights(dtype, tiles):
    """the shadow's compute-dtype weight copies are built by an eval pass BEFORE the updates; the updates write P through a raw
    pointer, so without ParamStore.mark_dirty() the next eval pass would use the stale copies"""
    from build_utils.parse_config import materialize_cfg
    from build_utils.torch_utils import ModelEMA
    from dyk.optim import FusedAdam
    from models import YOLO
    m = _model(dtype).train()
    ema = ModelEMA(m)
    x, y = _inputs()
    before = _heads(ema.ema, x, y)
    opt = FusedAdam(m, lr=1e-3, betas=(0.937, 0.999))
    for _ in range(2):
        _train_step(m, opt, x, y)
        ema.update(m)
    ema.update_attr(m)
    ema.ema.eval()
    got = _heads(ema.ema, x, y)
    fresh = YOLO(materialize_cfg(C2))
    fresh.load_state_dict(ema.ema.state_dict())
    fresh.dyk_dtype = dtype
    fresh = fresh.cuda().eval()
    want = _heads(fresh, x, y)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    assert not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, before))


def test_ema_does_not_disturb_training(tiles):
    from build_utils.torch_utils import ModelEMA
    from dyk.optim import FusedAdam
    x, y = _inputs()
    runs = []
    for with_ema in (False, True):
        m = _model().train()
        opt = FusedAdam(m, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
        ema = ModelEMA(m) if with_ema else None
        losses = []
        for _ in range(3):
            losses.append(_train_step(m, opt, x, y))
            if ema is not None:
                ema.update(m)
        runs.append((torch.stack(losses), _snapshot(m)))
    (l0, s0), (l1, s1) = runs
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    for k in s0:
        assert torch.equal(_bits(s0[k]), _bits(s1[k])), k


def test_deepcopy_after_forward_backward_and_step_is_independent(tiles):
    from dyk.optim import FusedAdam
    m = _model().train()
    x, y = _inputs()
    opt = FusedAdam(m, lr=1e-3, betas=(0.937, 0.999))
    _train_step(m, opt, x, y)
    out = m(x, y)                                  # and gradients left in the flat buffer
    sum((t ** 2).mean() for t in out).backward()
    m.eval()
    h0 = _heads(m, x, y)
    c = copy.deepcopy(m)
    assert c._engine is None and m._engine is not None
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_heads(c, x, y), h0))     # same values
    with torch.no_grad():
        for p in c.parameters():
            p.mul_(0.5)
    hc = _heads(c, x, y)
    assert not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(hc, h0))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_heads(m, x, y), h0))     # the original is untouched
    so, sc = m.engine.store, c.engine.store
    assert sc.P.data_ptr() != so.P.data_ptr() and sc.R.data_ptr() != so.R.data_ptr()
    mine = {a.tensor.data_ptr() for p in m.engine.plans.values() for a in p.arenas.values()}
    theirs = {a.tensor.data_ptr() for p in c.engine.plans.values() for a in p.arenas.values()}
    assert theirs and not (mine & theirs)
    # the copy trains on its own buffers
    c.train()
    _train_step(c, FusedAdam(c, lr=1e-3), x, y)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_heads(m, x, y), h0))


def test_ema_checkpoint_round_trip_is_bit_identical(tiles):
    from build_utils.parse_config import materialize_cfg
    from build_utils.torch_utils import ModelEMA
    from dyk.optim import FusedAdam
    from models import YOLO
    m = _model().train()
    x, y = _inputs()
    opt = FusedAdam(m, lr=1e-3, betas=(0.937, 0.999))
    ema = ModelEMA(m)
    buf = io.BytesIO()
    for i in range(3):
        _train_step(m, opt, x, y)
        if i == 2:
            torch.save({"ema": ema.ema.state_dict(), "updates": ema.updates}, buf)
        ema.update(m)
    # a new model holding the weights the third update saw, a new ModelEMA restored from the checkpoint of update 2
    m2 = YOLO(materialize_cfg(C2))
    m2.load_state_dict(m.state_dict())
    m2.dyk_dtype = "fp32"
    m2 = m2.cuda()
    buf.seek(0)
    ck = torch.load(buf, map_location="cpu")
    ema2 = ModelEMA(m2)
    ema2.ema.load_state_dict(ck["ema"])
    ema2.updates = ck["updates"]
    assert ema2.updates == 2
    ema2.update(m2)
    a, b = ema.ema.state_dict(), ema2.ema.state_dict()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
