"""dyk_anchor_assign, dyk_anchor_median and dyk_anchor_fitness on the device against the numpy restatement
tests/anchor_ref.py, BIT FOR BIT over tests/anchor_cases.py (nearest, counts, changed, the centres, all four fitness outputs),
on sentinel-framed buffers; the wrappers of other_utils/anchor_cluster.py (k_means, anchor_fitness, evolve_anchors for three
windows, anchor_cluster end to end) against the sequential restatement; the limits.  tests/test_anchor_reference.py ties the
restatement to the reference's recorded results."""
import ctypes
import random
import warnings

import numpy as np
import pytest
import torch

import anchor_cases as C
import anchor_ref as R

pytestmark = pytest.mark.gpu
GUARD, FILL = 256, 0xA5


class Framed:
    """a device buffer of `nbytes` between two guard zones filled with a sentinel"""

    def __init__(self, nbytes, init=None):
        self.n = nbytes
        self.buf = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device="cuda")
        if init is not None:
            self.buf[GUARD:GUARD + nbytes] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(init).tobytes(), np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == FILL).all() and (host[GUARD + self.n:] == FILL).all(), "a guard zone was written"
        return host[GUARD:GUARD + self.n].view(dtype).copy()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def device_step(wh, c):
    """one assign (against a zero-filled buffer), a second assign against its own result, one median -> what the device wrote"""
    from dyk import lib as L
    h = L.load()
    N, K, eb = len(wh), len(c), wh.dtype.itemsize
    dwh, dc = Framed(wh.nbytes, wh), Framed(c.nbytes, c)
    near, stats = Framed(4 * N, np.zeros(N, np.int32)), Framed(4 * (K + 2))
    da = L.DykAnchorAssignDesc(wh=dwh.ptr, c=dc.ptr, nearest=near.ptr, stats=stats.ptr, N=N, K=K, elem_bytes=eb)
    L.check(h.dyk_anchor_assign(ctypes.byref(da), _stream()), "dyk_anchor_assign")
    nearest, s1 = near.read(np.int32), stats.read(np.int32)
    L.check(h.dyk_anchor_assign(ctypes.byref(da), _stream()), "dyk_anchor_assign")
    nearest2, s2 = near.read(np.int32), stats.read(np.int32)
    ws = Framed(h.dyk_anchor_median_ws_bytes(K))
    dm = L.DykAnchorMedianDesc(wh=dwh.ptr, nearest=near.ptr, c=dc.ptr, ws=ws.ptr, ws_bytes=ws.n, N=N, K=K, elem_bytes=eb)
    L.check(h.dyk_anchor_median(ctypes.byref(dm), _stream()), "dyk_anchor_median")
    ws.read(np.uint8)
    assert np.array_equal(dwh.read(wh.dtype).reshape(wh.shape), wh) and np.array_equal(near.read(np.int32), nearest)
    return nearest, s1, nearest2, s2, dc.read(c.dtype).reshape(c.shape)


@pytest.mark.parametrize("T", C.DTYPES)
def test_assign_and_median_equal_the_restatement_bit_for_bit(T):
    cases = {n: v for n, v in C.assign_cases().items() if v[0].dtype == T}
    assert len(cases) > 30
    for name, (wh, c) in cases.items():
        K = len(c)
        ref_near, ref_counts, ref_changed = R.assign(wh, c)
        nearest, s1, nearest2, s2, centres = device_step(wh, c)
        assert np.array_equal(nearest, ref_near), name
        assert np.array_equal(s1[:K], ref_counts) and s1[K] == ref_changed and s1[K + 1] == 0, (name, s1.tolist())
        assert np.array_equal(nearest2, ref_near) and np.array_equal(s2[:K], ref_counts) and s2[K] == 0 and s2[K + 1] == 0, name
        assert np.array_equal(_bits(centres), _bits(R.median(wh, ref_near, c))), name


def device_fitness(wh, a, thr):
    from dyk import lib as L
    h = L.load()
    G, K, N = a.shape[0], a.shape[1], len(wh)
    need = h.dyk_anchor_fitness_ws_bytes(N, G, K)
    dwh, da, ws = Framed(wh.nbytes, wh), Framed(a.nbytes, a), Framed(need)
    outs = [Framed(8 * G), Framed(8 * G), Framed(4 * G), Framed(4 * G)]
    d = L.DykAnchorFitnessDesc(wh=dwh.ptr, a=da.ptr, ws=ws.ptr, fit_boxes=outs[0].ptr, fit_anchors=outs[1].ptr, hit_boxes=outs[2].ptr,
                               hit_anchors=outs[3].ptr, ws_bytes=need, thr=thr, N=N, K=K, G=G, elem_bytes=wh.dtype.itemsize)
    L.check(h.dyk_anchor_fitness(ctypes.byref(d), _stream()), "dyk_anchor_fitness")
    ws.read(np.uint8)
    return {"fit_boxes": outs[0].read(np.float64), "fit_anchors": outs[1].read(np.float64), "hit_boxes": outs[2].read(np.int32),
            "hit_anchors": outs[3].read(np.int32)}


@pytest.mark.parametrize("T", C.DTYPES)
def test_fitness_equals_the_restatement_bit_for_bit_and_repeats(T):
    cases = {n: v for n, v in C.fitness_cases().items() if v[0].dtype == T}
    assert len(cases) > 25
    for name, (wh, a, thr) in cases.items():
        ref = R.fitness_batch(wh, a, thr)
        one, two = device_fitness(wh, a, thr), device_fitness(wh, a, thr)
        for key in ("fit_boxes", "fit_anchors"):
            assert np.array_equal(_bits(one[key]), _bits(np.asarray(ref[key], np.float64))), (name, key, one[key][:4], ref[key][:4])
            assert np.array_equal(_bits(one[key]), _bits(two[key])), (name, key)
        for key in ("hit_boxes", "hit_anchors"):
            assert np.array_equal(one[key], ref[key]) and np.array_equal(one[key], two[key]), (name, key)


def test_fitness_of_a_candidate_does_not_depend_on_the_batch():
    wh, a = C.boxes(4099, np.float32), C.candidates(9, 64)
    whole = device_fitness(wh, a, C.THR)
    for g in (0, 13, 63):
        alone = device_fitness(wh, a[g:g + 1], C.THR)
        for key in whole:
            assert alone[key][0] == whole[key][g], (g, key)


# ------------------------------------------------------------------------------------------------ the wrappers
def test_k_means_wrapper_equals_the_restatement():
    from other_utils import anchor_cluster as A
    for name, (wh, init) in C.kmeans_cases().items():
        ref, iters, empties = R.k_means(wh, init=init)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            info = {}
            got = A.k_means(wh, len(init), init=init, info=info)
        assert isinstance(got, np.ndarray) and got.dtype == wh.dtype and np.array_equal(_bits(got), _bits(ref)), name
        assert info == {"iterations": iters, "readbacks": iters, "entry_calls": 2 * iters - 1}, (name, info)
        said = [str(x.message) for x in w if "no member" in str(x.message)]
        assert len(said) == (1 if empties else 0) and all(str(j) in said[0] for j in empties), (name, said)
    wh = C.boxes(257, np.float32)
    np.random.seed(1)
    ref = R.k_means(wh, 9)[0]
    np.random.seed(1)
    got = A.k_means(torch.from_numpy(wh).cuda(), 9)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), ref)


def test_anchor_fitness_and_evolution_equal_the_sequential_chain():
    from other_utils import anchor_cluster as A
    wh = C.boxes(257, np.float32)
    k0 = R.k_means(wh, init=C.centres(wh, 9))[0]
    ref = R.fitness(wh, k0.astype(np.float64), C.THR)
    f, br = A.anchor_fitness(wh, k0, C.THR)
    assert f == ref["fit_boxes"] and br == ref["hit_boxes"] / 257.0
    for kind, windows in (("boxes", (1, 7, 64)), ("reference", (7,))):
        random.seed(21)
        np.random.seed(22)
        rk, rf, rn = R.evolve(wh, k0, C.THR, 50, kind)
        for window in windows:
            random.seed(21)
            np.random.seed(22)
            info = {}
            k, f, n = A.evolve_anchors(wh, k0, thr=C.THR, gen=50, fitness=kind, window=window, info=info)
            assert np.array_equal(_bits(k), _bits(rk)) and f == rf and n == rn, (kind, window, n, rn)
            # one launch for the starting fitness, then per launch either an accept or a whole window without one
            assert info["accepted"] == n and info["readbacks"] == info["launches"] <= (51 if window == 1 else 2 + n + 50 // window)
        if kind == "boxes":
            assert rn > 0 and rf > ref["fit_boxes"]


def test_anchor_cluster_end_to_end_equals_the_restatement_chain(capsys):
    from other_utils import anchor_cluster as A
    wh0 = np.concatenate([C.boxes(257, np.float32, seed=31), np.array([[1.5, 1.2], [2.5, 1.0], [1.0, 1.9]], np.float32)])
    for kind in A.FITNESS_KINDS:
        random.seed(41)
        np.random.seed(42)
        rk, rf = R.cluster(wh0, 9, C.THR, 30, kind)
        random.seed(41)
        np.random.seed(42)
        k = A.anchor_cluster(n=9, thr=C.THR, gen=30, wh=wh0, fitness=kind)
        out = capsys.readouterr().out
        assert k.dtype == np.float64 and np.array_equal(_bits(k), _bits(rk)), kind
        assert "WARNING: Extremely small objects found. 3 of 260" in out and "kmeans: [" in out and "genetic: [" in out
        assert ("fitness: %.5f" % rf) in out


def test_the_limits_raise():
    from other_utils import anchor_cluster as A
    wh = C.boxes(65, np.float32)
    for bad, exc in ((wh.astype(np.float16), TypeError), (wh.astype(np.int32), TypeError), (wh[:, ::-1], ValueError), (wh[:, :1], ValueError),
                     (wh.reshape(-1), ValueError), (wh[:0], ValueError), (list(wh), TypeError), (torch.from_numpy(wh), TypeError)):
        with pytest.raises(exc):
            A.k_means(bad, 1)
        with pytest.raises(exc):
            A.anchor_fitness(bad, wh[:3], C.THR)
    for v in (0.0, -1.0, np.nan, np.inf):
        broken = wh.copy()
        broken[7, 1] = v
        with pytest.raises(ValueError):
            A.k_means(broken, 3)
        with pytest.raises(ValueError, match="1 of the 65"):
            A.k_means(torch.from_numpy(broken).cuda(), 3)                    # counted by the assignment launch
        with pytest.raises(ValueError):
            A.anchor_fitness(wh, broken[:9], C.THR)
    for k in (0, 33):
        with pytest.raises(ValueError):
            A.k_means(wh, k)
    with pytest.raises(ValueError):
        A.k_means(wh, 66)                                                    # above the limit of 32
    for few in (wh[:8].copy(), torch.from_numpy(wh[:8].copy()).cuda()):
        with pytest.raises(ValueError, match="at least as many boxes"):
            A.k_means(few, 9)                                                # within the limit, but more clusters than boxes
    broken = wh.copy()
    broken[3, 0] = -2.0
    dev = torch.from_numpy(broken).cuda()
    for call in (lambda: A.anchor_fitness(dev, wh[:3], C.THR), lambda: A.evolve_anchors(dev, wh[:3], gen=2),
                 lambda: A.fitness_batch(dev, wh[:3], C.THR)):
        with pytest.raises(ValueError, match="1 of the 65"):                 # device boxes: counted by an assignment launch
            call()
    with pytest.raises(ValueError):
        A.anchor_fitness(wh, C.candidates(33, 1)[0], C.THR)
    with pytest.raises(ValueError):
        A.fitness_batch(wh, C.candidates(2, 4097), C.THR)
    with pytest.raises(ValueError):
        A.anchor_fitness(wh, wh[:3], float("nan"))
    with pytest.raises(ValueError):
        A.evolve_anchors(wh, wh[:3], window=4097)
