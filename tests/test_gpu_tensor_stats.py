"""dyk_tensor_stats (csrc/tensor_stats.hip) at its own ABI on synthetic tables -- exact absmax / counts, sumsq bit for bit against
the numpy restatement of the documented order and within the derived bound of the plain fp64 reference (tests/tensor_stats_ref.py),
NaN between the segments, sentinel-framed workspace and output -- and dyk.monitor.TensorStats on the smallest model that trains
(the cfg and helpers of tests/test_gpu_harness.py, 2 image pairs of 64 x 64, autotuner off)."""
import math

import numpy as np
import pytest
import torch

import tensor_stats_ref as R
from helpers import C1
from test_gpu_harness import _backward, _batch, _model

pytestmark = pytest.mark.gpu

_CACHE = {}
FRAME = 96


def _case(key):
    """(bufs, segments, plain reference, restatement), computed once per process and shared (do not modify)"""
    if key not in _CACHE:
        if key[0] == "long":
            numel = key[1]
            rng = np.random.default_rng(numel)
            buf = np.full(numel + 72, np.nan, np.float32)
            buf[8:8 + numel] = (1.0 + rng.random(numel)).astype(np.float32)
            bufs, segments = [buf], [(8, numel, 0)]
        else:
            bufs, segments = R.kernel_case(*key)
        _CACHE[key] = (bufs, segments, R.plain_reference(bufs, segments), R.restate(bufs, segments))
    return _CACHE[key]


def _run(bufs, segments):
    """one dyk_tensor_stats call on fresh device copies -> (STAT[nseg][nbuf], raw output bytes); workspace and output stand
    between guard bands of 0xa5 and are filled with it"""
    from dyk import ops
    dev = torch.device("cuda", 0)
    table = ops.tensor_stats_worklist(segments, dev)
    nseg, nbuf = len(segments), len(bufs)
    assert table["nseg"] == nseg and table["nitems"] == sum(R.items_of(n) for _, n, _ in segments)
    need = int(ops.load().dyk_tensor_stats_ws_bytes(table["nitems"], nbuf))
    assert need == 24 * table["nitems"] * nbuf
    ws = torch.full((need + 2 * FRAME,), 0xa5, dtype=torch.uint8, device=dev)
    nout = nseg * nbuf * ops.TSTAT_BYTES
    out = torch.full((nout + 2 * FRAME,), 0xa5, dtype=torch.uint8, device=dev)
    dbufs = [torch.from_numpy(b).to(dev) for b in bufs]
    ops.tensor_stats(dbufs, table, out[FRAME:FRAME + nout], ws[FRAME:FRAME + need])
    torch.cuda.synchronize()
    for name, t, n in (("workspace", ws, need), ("output", out, nout)):
        assert bool((t[:FRAME] == 0xa5).all()) and bool((t[FRAME + n:] == 0xa5).all()), "a kernel wrote outside its %s" % name
    for b, d in zip(bufs, dbufs):
        assert d.cpu().numpy().tobytes() == b.tobytes(), "a buffer was written"
    raw = out[FRAME:FRAME + nout].cpu().numpy().tobytes()
    return ops.tensor_stats_records(raw, nseg, nbuf), raw


CASES = [("store", 1, False, False), ("packed", 2, True, False), ("mixed", 3, False, True), ("mixed", 4, True, True),
         ("packed", 4, False, False), ("store", 2, True, True), ("long", 69 * 4096 + 77), ("long", 130 * 4096 + 5)]


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(str(x) for x in k))
def test_kernel_against_the_restatement_and_fp64(key):
    bufs, segments, ref, want = _case(key)
    rec, raw = _run(bufs, segments)
    for s, (off, numel, flags) in enumerate(segments):
        for k in range(len(bufs)):
            r, w = rec[s, k], ref[s][k]
            if w is not None and w["norm"] > 0:
                print("seg %2d numel %6d buf %d: norm rel err %.3g (bound %.3g) absmax %g nonfinite %d zeros %d" % (
                    s, numel, k, abs(math.sqrt(r["sumsq"]) - w["norm"]) / w["norm"], R.norm_bound(numel), r["absmax"],
                    r["nonfinite"], r["zeros"]))
    assert R.deviations(rec, bufs, segments, ref) == []                     # exact absmax / counts, norm within the bound, skips zeroed
    assert np.array_equal(rec["sumsq"].view(np.uint64), want["sumsq"].view(np.uint64)), "sumsq is not the documented order's"
    assert raw == want.tobytes()
    _, raw2 = _run(bufs, segments)
    assert raw2 == raw, "two runs of the same reduction differ"


def test_special_values_are_where_the_cases_say():
    """the special-value cases hold what they claim: inf / NaN / -0.0 / a denormal / FLT_MAX at the first and last element of a
    segment and on both sides of an item boundary, and the device counts each of them"""
    bufs, segments, ref, _ = _case(("packed", 2, True, False))
    b = bufs[0]
    off, numel, _ = segments[-1]
    assert numel == 3 * 4096 + 1
    spots = R.special_spots(off, numel)
    assert [p - off for p in spots] == [0, 4095, 4096, 8191, 8192, 12287, 12288]
    planted = b[spots]
    assert np.isnan(planted).any() and np.isinf(planted).any()
    everything = np.concatenate([bb[o:o + n] for bb in bufs for o, n, _ in segments])
    assert np.any(everything == np.float32(R.F32_MAX)) and np.any((everything == 0) & np.signbit(everything))
    assert np.any((everything != 0) & (np.abs(everything) < np.finfo(np.float32).tiny))
    rec, _ = _run(bufs, segments)
    for s, (o, n, _) in enumerate(segments):
        for k, bb in enumerate(bufs):
            x = bb[o:o + n]
            assert rec[s, k]["nonfinite"] == np.count_nonzero(~np.isfinite(x)) and rec[s, k]["zeros"] == np.count_nonzero(x == 0)
    assert sum(int(r["nonfinite"]) for r in rec.ravel()) > 8 and sum(int(r["zeros"]) for r in rec.ravel()) > 2


def test_buffer_count_does_not_change_a_record():
    """the records of buffer k are the same bits whether it is reduced alone or beside others"""
    bufs, segments, _, _ = _case(("packed", 4, False, False))
    all4, _ = _run(bufs, segments)
    for k in (0, 3):
        alone, _ = _run([bufs[k]], segments)
        assert alone[:, 0].tobytes() == all4[:, k].tobytes()


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def trained():
    """the model after one forward + loss + backward, and its batch"""
    mp = pytest.MonkeyPatch()
    mp.setenv("DYK_AUTOTUNE", "0")
    mp.setenv("DYK_TUNE_CACHE", "0")
    try:
        m = _model(C1)
        batch = _batch(5, B=2, H=64, W=64)
        _backward(m, batch)
        yield m, batch
    finally:
        mp.undo()


def _again(m, batch):
    m.engine.store.G.zero_()
    _backward(m, batch)


def _torch_stats(tensors):
    """per tensor, the torch way: (double norm, abs max, non-finite count, zero count), one synchronisation for all"""
    rows = []
    for t in tensors:
        t = t.detach()
        fin = torch.isfinite(t)
        tf = torch.where(fin, t, torch.zeros_like(t))
        rows.append(torch.stack([tf.double().norm(), tf.abs().max().double(), (~fin).sum().double(), (t == 0).sum().double()]))
    return torch.stack(rows).cpu().numpy()


def _check_against_torch(stats, named):
    """{name: Stat} against the tensors [(name, tensor)]"""
    assert list(stats) == [n for n, _ in named]
    ref = _torch_stats([t for _, t in named])
    worst = 0.0
    for (name, t), (norm, amax, bad, zeros) in zip(named, ref):
        s = stats[name]
        assert s.numel == t.numel()
        assert (s.absmax, s.nonfinite, s.zeros) == (amax, int(bad), int(zeros)), name
        bound = R.other_order_bound(s.numel)
        assert abs(s.norm - norm) <= bound * norm, (name, s.norm, norm, bound)
        assert abs(float(np.float32(s.norm)) - norm) <= 2.0 ** -23 * norm, name
        if norm > 0:
            worst = max(worst, abs(s.norm - norm) / norm)
    print("%d tensors, worst relative norm error %.3g" % (len(named), worst))


def test_param_and_grad_agree_with_torch_per_parameter(trained):
    from dyk.monitor import TensorStats
    m, batch = trained
    _again(m, batch)
    ts = TensorStats(m, what=("param", "grad"))
    ts.launch()
    r = ts.read(wait=True)
    assert sorted(r) == ["grad", "param"]
    named = list(m.named_parameters())
    assert list(r["param"]) == list(r["grad"]) == [n for n, _ in named]
    _check_against_torch(r["param"], named)
    _check_against_torch(r["grad"], [(n, p.grad) for n, p in named])
    assert sum(s.norm > 0 for s in r["grad"].values()) > len(named) // 2
    assert ts.first_nonfinite() == []
    text = ts.summary(k=3)
    assert "largest norm" in text and "no non-finite" in text and len(text.splitlines()) < 16


def test_summed_sumsq_agrees_with_the_guard_norm(trained):
    from dyk.monitor import TensorStats
    from dyk.optim import FusedAdam
    m, batch = trained
    _again(m, batch)
    p0 = m.engine.store.P.clone()
    ts = TensorStats(m)
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=1e9)
    assert opt.grad_scale == 1.0
    ts.launch()
    opt.step()
    r = ts.read(wait=True)["grad"]
    guard = opt.grad_stats(wait=True)["norm"]
    total = math.sqrt(math.fsum(s.sumsq for s in r.values()))
    # ours: every tensor's sumsq within gamma(K) of exact, so is their exact sum (fsum), the root halves it; the guard's norm is
    # within 2^-23 of exact (tests/grad_guard_ref.py)
    bound = 2.0 ** -23 + R.gamma(max(R.roundings(s.numel) for s in r.values())) / 2 + 4 * R.U
    print("sum of per-tensor sumsq -> %.17g, guard %.9g, rel %.3g (bound %.3g)" % (total, guard, abs(total - guard) / guard, bound))
    assert guard > 0 and abs(total - guard) <= bound * guard
    with torch.no_grad():
        m.engine.store.P.copy_(p0)                   # (leave the shared model as it was)
    m.engine.store.mark_dirty()


def test_one_inf_names_its_tensor_and_leaves_the_others_alone(trained):
    from dyk.monitor import TensorStats
    m, batch = trained
    _again(m, batch)
    ts = TensorStats(m, what=("grad",))
    ts.launch()
    before = ts.read(wait=True)["grad"]
    names = [n for n, _ in m.named_parameters()]
    victim_name = names[len(names) // 3]
    victim = dict(m.named_parameters())[victim_name]
    idx = tuple(d - 1 for d in victim.grad.shape)
    old = victim.grad[idx].clone()
    victim.grad[idx] = float("inf")                              # one element of one gradient view
    ts.launch()
    assert ts.first_nonfinite() == [victim_name]
    after = ts.read(wait=True)["grad"]
    assert after[victim_name].nonfinite == 1 and math.isfinite(after[victim_name].norm)
    for n in names:
        if n != victim_name:
            assert after[n] == before[n], n                      # (all fields are non-negative numbers: == is bit equality)
    assert victim_name in ts.summary()
    # two tensors: reverse store order, the deeper one first
    other = names[len(names) // 3 - 2]
    og = dict(m.named_parameters())[other].grad
    og[(0,) * og.dim()] = float("nan")
    ts.launch()
    assert ts.first_nonfinite() == [victim_name, other]
    victim.grad[idx] = old


def test_a_frozen_parameter_is_reported_for_param_only(trained):
    from dyk.monitor import TensorStats
    m, batch = trained
    named = list(m.named_parameters())
    name, p = named[-3]
    ts = TensorStats(m, what=("grad", "param"))
    try:
        p.requires_grad_(False)
        m.engine.store.G.zero_()
        _backward(m, batch)
        ts.launch()
        r = ts.read(wait=True)
        assert list(r["param"]) == [n for n, _ in named]
        assert list(r["grad"]) == [n for n, _ in named if n != name]
        want = float(p.detach().double().norm())
        assert abs(r["param"][name].norm - want) <= R.other_order_bound(p.numel()) * want and want > 0
    finally:
        p.requires_grad_(True)
    _again(m, batch)
    ts.launch()
    assert name in ts.read(wait=True)["grad"]


def test_adam_moments_match_the_exported_state(trained):
    from dyk.monitor import TensorStats
    from dyk.optim import FusedAdam
    m, batch = trained
    _again(m, batch)
    st = m.engine.store
    p0 = st.P.clone()
    opt = FusedAdam(m, lr=1e-4)
    with pytest.raises(Exception, match="no exp_avg yet"):
        TensorStats(m, what=("exp_avg",), optimizer=opt).launch()
    opt.step()
    ts = TensorStats(m, what=("exp_avg", "exp_avg_sq", "running"), optimizer=opt)
    ts.launch()
    r = ts.read(wait=True)
    opt._export_state()
    named = list(m.named_parameters())
    for key in ("exp_avg", "exp_avg_sq"):
        _check_against_torch(r[key], [(n, opt.state[p][key]) for n, p in named])
        assert sum(s.norm > 0 for s in r[key].values()) > len(named) // 2
    opt.state.clear()
    running = [(n, b) for n, b in m.named_buffers() if n.endswith(("running_mean", "running_var"))]
    _check_against_torch(r["running"], running)
    with torch.no_grad():
        st.P.copy_(p0)
    st.mark_dirty()


def test_read_without_waiting_is_none_or_complete(trained):
    from dyk.monitor import TensorStats
    m, batch = trained
    names = [n for n, _ in m.named_parameters()]
    ts = TensorStats(m, what=("grad", "param"))
    assert ts.read() is None
    seen = 0
    for _ in range(12):                              # more launches than the ring has slots
        ts.launch()
        r = ts.read(wait=False)
        if r is not None:
            seen += 1
            assert list(r["grad"]) == names and list(r["param"]) == names
            assert all(s.numel > 0 and s.norm >= 0 for s in r["param"].values())
    r = ts.read(wait=True)
    assert r is not None and list(r["grad"]) == names and not ts._pending
    print("results seen without waiting: %d of 12" % seen)
