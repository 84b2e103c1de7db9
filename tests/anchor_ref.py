"""Plain numpy restatement of the anchor-clustering rule of include/dyk_hip.h (dyk_anchor_assign, dyk_anchor_median,
dyk_anchor_fitness) and of the sequential k-means and evolution loops of other_utils/anchor_cluster.py.  The yardstick of
tests/test_anchor_reference.py (held to the reference's recorded results and to hand-worked cases) and of
tests/test_gpu_anchor_cluster.py (the device entries equal it bit for bit).  numpy rounds every elementwise operation on its
own and never contracts, which is the rule; the one order-dependent quantity, the fp64 sum of the "boxes" fitness, is added
in the header's order.  Every function takes `variant=`: None is the rule, a name is one deliberately wrong reading of it,
used by the tests to show that the named cases tell them apart."""
import random

import numpy as np

FIT_ITEM, BLOCK, WAVE = 1024, 256, 64


# ------------------------------------------------------------------------------------------------ assignment
def distances(wh, c, variant=None):
    """d[i][k] = 1 - iou in the type of the inputs, each operation rounded on its own"""
    assert wh.dtype == c.dtype and wh.dtype in (np.float32, np.float64)
    T = wh.dtype.type
    w, h, cw, ch = wh[:, None, 0], wh[:, None, 1], c[None, :, 0], c[None, :, 1]
    inter = np.minimum(w, cw) * np.minimum(h, ch)
    if variant == "fma_denominator":
        # (w * h) + (cw * ch) with the second product unrounded: fma(cw, ch, w * h), formed exactly in a wider type
        wide = np.longdouble if T is np.float64 else np.float64
        s = ((w * h).astype(wide) + cw.astype(wide) * ch.astype(wide)).astype(T)
        union = s - inter
    else:
        union = ((w * h) + (cw * ch)) - inter
    iou = inter / union
    if variant == "argmax_iou":
        return -iou
    return T(1) - iou


def assign(wh, c, prev=None, variant=None):
    """-> (nearest int32 [N], counts int32 [K], changed): the first minimum of d; `changed` against prev (zeros when None)"""
    d = distances(wh, c, variant)
    if variant == "last_minimum":
        nearest = (d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)).astype(np.int32)
    else:
        nearest = np.argmin(d, axis=1).astype(np.int32)
    prev = np.zeros(len(wh), np.int32) if prev is None else prev
    return nearest, np.bincount(nearest, minlength=len(c)).astype(np.int32), int((nearest != prev).sum())


# ------------------------------------------------------------------------------------------------ median
def median(wh, nearest, c, variant=None):
    """-> new centres: per cluster and coordinate the median of the members, an empty cluster keeps its centre"""
    T = wh.dtype.type
    out = c.copy()
    for k in range(len(c)):
        mem = wh[nearest == k]
        m = len(mem)
        if m == 0:
            if variant == "empty_zero":
                out[k] = 0
            elif variant == "empty_nan":
                out[k] = np.nan
            continue
        if variant == "median_area_member":
            order = np.argsort(mem[:, 0] * mem[:, 1], kind="stable")
            out[k] = mem[order[(m - 1) // 2]]
            continue
        for j in range(2):
            x = np.sort(mem[:, j])
            if m & 1 or variant == "lower_middle":
                out[k, j] = x[(m - 1) // 2]
            else:
                out[k, j] = (x[m // 2 - 1] + x[m // 2]) / T(2)
    return out


def k_means(wh, k=None, init=None, variant=None, max_iter=10000):
    """The loop of other_utils.anchor_cluster.k_means: initial centres `init`, or k boxes drawn with np.random.choice.
    -> (centres, iterations, empties seen)"""
    c = (wh[np.random.choice(len(wh), k, replace=False)] if init is None else init).copy()
    nearest = np.zeros(len(wh), np.int32)
    empties = set()
    for it in range(1, max_iter + 1):
        nearest, counts, changed = assign(wh, c, nearest, variant)
        if changed == 0:
            return c, it, sorted(empties)
        empties.update(int(j) for j in np.nonzero(counts == 0)[0])
        c = median(wh, nearest, c, variant)
    raise RuntimeError("k_means did not settle in %d iterations" % max_iter)


# ------------------------------------------------------------------------------------------------ fitness
def ratio_matrix(wh, a, variant=None):
    """x[i][k] in fp64: min over the two coordinates of min(r, 1 / r), r = wh / a"""
    wh = wh.astype(np.float64)
    r = wh[:, None, :] / a[None, :, :]
    q = a[None, :, :] / wh[:, None, :] if variant == "a_over_w" else 1.0 / r
    return np.minimum(r, q).min(2)


def _lane_fold(v):
    """[..., 64] -> [...]: l += l+32, l+16, ..., l+1; lane 0 holds the result"""
    v = v.copy()
    off = WAVE // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def ordered_sum(term):
    """The fp64 sum of term[N] (all >= 0) in the order of dyk_anchor_fitness"""
    n = len(term)
    items = -(-n // FIT_ITEM)
    t = np.zeros(items * FIT_ITEM, np.float64)
    t[:n] = term
    t = t.reshape(items, FIT_ITEM // BLOCK, BLOCK // WAVE, WAVE)      # box = 1024 p + 256 u + 64 wave + lane
    acc = np.zeros(t[:, 0].shape, np.float64)
    for u in range(t.shape[1]):
        acc = acc + t[:, u]                                          # the thread's boxes in order
    w = _lane_fold(acc)                                              # [items, 4]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    rows = -(-items // WAVE)
    p = np.zeros(rows * WAVE, np.float64)
    p[:items] = part
    p = p.reshape(rows, WAVE)
    lane = np.zeros(WAVE, np.float64)
    for r in range(rows):
        lane = lane + p[r]                                           # lane l: items l, l + 64, ... in order
    return _lane_fold(lane)


def fitness(wh, a, thr, variant=None):
    """One candidate a[K,2] (fp64).  -> dict fit_boxes, hit_boxes, fit_anchors, hit_anchors"""
    a = np.asarray(a, np.float64)
    x = ratio_matrix(wh, a, variant)
    over = (lambda v: v >= thr) if variant == "ge_thr" else (lambda v: v > thr)
    b = x.max(1)
    fb = ordered_sum(np.where(over(b), b, 0.0)) / float(len(wh))
    t = x.max(0)
    s = 0.0
    for k in range(len(a)):
        s = s + (t[k] if over(t[k]) else 0.0)
    return {"fit_boxes": fb, "hit_boxes": int(over(b).sum()), "fit_anchors": s / float(len(a)), "hit_anchors": int(over(t).sum())}


def fitness_batch(wh, cands, thr):
    res = [fitness(wh, a, thr) for a in cands]
    return {key: np.array([r[key] for r in res]) for key in res[0]}


# ------------------------------------------------------------------------------------------------ evolution
def draw_factors(shape, gen, mp=0.9, sigma=0.1):
    """Per generation: a uniform array against mp, one scalar from `random`, a normal array, in that order; again while all
    factors are 1"""
    out = []
    for _ in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            keep = np.random.random(shape) < mp
            u = random.random()
            z = np.random.randn(*shape)
            v = np.clip(keep * u * z * sigma + 1, 0.3, 3.0)
        out.append(v)
    return np.array(out, np.float64).reshape((gen,) + tuple(shape))


def evolve(wh, k, thr=0.25, gen=1000, kind="boxes", factors=None, variant=None):
    """The sequential chain, one fitness per generation.  -> (anchors fp64, fitness, accepted)"""
    key = "fit_boxes" if kind == "boxes" else "fit_anchors"
    k = np.asarray(k, np.float64).copy()
    f = fitness(wh, k, thr)[key]
    v = draw_factors(k.shape, gen) if factors is None else factors
    accepted = 0
    for g in range(gen):
        kg = np.clip(k * v[g], 2.0, None)
        fg = fitness(wh, kg, thr)[key]
        if (fg >= f) if variant == "accept_ge" else (fg > f):
            f, k = fg, kg
            accepted += 1
    return k, f, accepted


def cluster(wh0, n, thr, gen, kind="boxes"):
    """anchor_cluster(wh=...) as a chain of the pieces above"""
    wh = np.ascontiguousarray(wh0[(wh0 >= 2.0).any(1)])
    k = k_means(wh, n)[0]
    k = k[np.argsort(k.prod(1))]
    k, f, _ = evolve(wh, k, thr, gen, kind)
    return k[np.argsort(k.prod(1))], f
