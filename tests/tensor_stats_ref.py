"""numpy restatement of the per-tensor statistics of csrc/tensor_stats.hip (dyk_tensor_stats) -- the work list, the ORDER of every
addition of the partials and fold kernels -- plus the plain fp64 reference the tests hold the device to, the synthetic tables
both test files use and a list of WRONG kernels the cases must flag.  Shared by tests/test_tensor_stats_reference.py (CPU) and
tests/test_gpu_tensor_stats.py; not an oracle of the reference project.

Order (include/dyk_hip.h): every segment is cut, in table order, into items of 4096 elements (the last one shorter).  One
workgroup of 256 threads per item: thread t takes the 16-byte vectors t, t + 256, t + 512, t + 768 of the item in that order,
the four elements of a vector in order, and adds x*x (an exact 0 for a non-finite x or an element past the item's length) to
an fp64 accumulator that starts at 0; 64 lanes fold as l += l+32, l+16, ..., l+1; the four waves add in order.  Fold: one wave
per segment, lane l adds the item partials l, l + 64, l + 128, ... of the segment in that order, the lanes fold as above.

Error of that order against the exact sum.  Every x*x is exact in fp64 (two 24-bit significands) and every term is >= 0, so
an addition has relative error <= u = 2^-53 and adding an exact zero has none.  A term passes through at most
    K(c) = 16 (a thread's elements) + 6 (lanes) + 3 (waves) + ceil(c / 64) (a fold lane's partials) + 6 (lanes)
rounding additions, c = ceil(numel / 4096) the items of its segment, hence
    |sumsq - exact| <= ((1 + u)^K - 1) * exact <= gamma(K) * exact,    gamma(K) = K u / (1 - K u)
(K = 49 for the largest tensor of the target cfg, 512 x 1024 x 3 x 3: 1152 items).  The root halves a relative error (to first
order; the second-order term is below u) and is rounded once:  |norm - sqrt(exact)| <= (gamma(K) / 2 + 2 u) * sqrt(exact).
The reference side: numpy's pairwise np.sum of n exact squares passes a term through at most 16 + 3 additions inside a leaf of
128 elements and ceil(log2(n / 128)) above it, P(n) = 19 + max(0, ceil(log2(n)) - 7) in all, and its root is rounded once more:
    |norm - norm_ref| <= (gamma(K) / 2 + gamma(P) / 2 + 4 u) * norm_ref  =: norm_bound(numel)
A reference summed in another order (torch's .double().norm() on the device) is covered by P = n - 1, the bound of ANY order
of n non-negative terms: other_order_bound(n).  After rounding the norm to fp32 (2^-24 more) all of these stay below 2^-23
for n < 2^28."""
import math

import numpy as np

ITEM = 4096
BLOCK = 256
WAVE = 64
VECS = ITEM // 4 // BLOCK          # vectors per thread: 4
U = 2.0 ** -53
F32_MAX = float(np.finfo(np.float32).max)

SEG = np.dtype([("offset", "<i8"), ("numel", "<i8"), ("flags", "<u4"), ("item_begin", "<i4")])
ITEM_T = np.dtype([("first", "<i8"), ("seg", "<i4"), ("len", "<i4")])
STAT = np.dtype([("sumsq", "<f8"), ("absmax", "<f4"), ("nonfinite", "<u4"), ("zeros", "<u4"), ("_pad", "<u4")])


# ------------------------------------------------------------------ bounds
def gamma(k):
    return k * U / (1.0 - k * U)


def items_of(numel):
    return (numel + ITEM - 1) // ITEM


def roundings(numel):
    """K(c): the rounding additions a term of a segment of `numel` elements passes through on the device"""
    return 16 + 6 + 3 + (items_of(numel) + WAVE - 1) // WAVE + 6


def sumsq_bound(numel):
    """relative, against the EXACT sum"""
    return gamma(roundings(numel))


def pairwise_roundings(n):
    return 19 + max(0, int(math.ceil(math.log2(max(n, 1)))) - 7)


def norm_bound(numel):
    """relative, the device's sqrt(sumsq) against sqrt(np.sum(x*x)) of plain_reference"""
    return gamma(roundings(numel)) / 2 + gamma(pairwise_roundings(numel)) / 2 + 4 * U


def other_order_bound(numel):
    """the same against a root of a sum of the squares taken in an unknown order (a device reduction)"""
    return gamma(roundings(numel)) / 2 + gamma(max(numel - 1, 1)) / 2 + 4 * U


# ------------------------------------------------------------------ work list
def work_list(segments):
    """[(offset, numel, flags)] -> (DykTensorSeg[nseg], DykTensorItem[nitems]), built one item at a time (the vectorised
    builder of dyk/ops.py is held to this one)"""
    segs = np.zeros(len(segments), SEG)
    items = []
    for s, (off, numel, flags) in enumerate(segments):
        assert off % 4 == 0 and off >= 0 and numel >= 1
        segs[s] = (off, numel, flags, len(items))
        done = 0
        while done < numel:
            ln = min(ITEM, numel - done)
            items.append((off + done, s, ln))
            done += ln
    return segs, np.array(items, ITEM_T)


# ------------------------------------------------------------------ the documented order
def _lane_fold(a):
    """[..., 64] -> [...]: l += l+32, l+16, ..., l+1"""
    a = a.copy()
    off = WAVE // 2
    while off:
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def _classify(x, live, zlive, wrong):
    """per element: (square that is added, magnitude that enters the max, non-finite, zero)"""
    ax = np.abs(x)
    with np.errstate(all="ignore"):
        fin = ax <= np.float32(F32_MAX)
        keep = live & fin if wrong != "inf_taken" else live
        xd = np.where(keep, ax, np.float32(0)).astype(np.float64)
        sq = xd * xd
    return sq, np.where(keep, ax, np.float32(0)), live & ~fin, zlive & (ax == 0)


def partials(buf, items, wrong=None):
    """one buffer -> STAT[nitems], exactly what the partials kernel leaves in its workspace (`wrong`: one of WRONG_KERNELS)"""
    buf = np.asarray(buf, np.float32)
    n_items = len(items)
    idx = items["first"][:, None] + np.arange(ITEM)[None, :]
    ln = items["len"].astype(np.int64)
    if wrong == "tail_vector_whole":
        ln = (ln + 3) // 4 * 4
    live = np.arange(ITEM)[None, :] < ln[:, None]
    x = np.where(idx < len(buf), buf[np.minimum(idx, len(buf) - 1)], np.float32(0))      # (never read by the kernel: masked below)
    zlive = live
    if wrong == "padding_in_zeros":          # (zeros counted over the whole tail vector)
        zlive = np.arange(ITEM)[None, :] < ((items["len"].astype(np.int64) + 3) // 4 * 4)[:, None]
    sq, mag, bad, zero = _classify(x, live, zlive, wrong)
    # element 4 * (t + 256 u) + j  ->  [item][u][t][j]
    sq = sq.reshape(n_items, VECS, BLOCK, 4)
    acc = np.zeros((n_items, BLOCK))
    for u in range(VECS):
        for j in range(4):
            acc = acc + sq[:, u, :, j]
    waves = _lane_fold(acc.reshape(n_items, BLOCK // WAVE, WAVE))
    tot = waves[:, 0]
    for w in range(1, BLOCK // WAVE):
        tot = tot + waves[:, w]
    out = np.zeros(n_items, STAT)
    out["sumsq"] = tot
    out["absmax"] = mag.max(axis=1)
    out["nonfinite"] = bad.sum(axis=1)
    out["zeros"] = zero.sum(axis=1)
    return out


def fold(parts, segs, k, wrong=None):
    """STAT[nitems] of buffer k -> STAT[nseg]: the fold kernel"""
    out = np.zeros(len(segs), STAT)
    for s, sg in enumerate(segs):
        if (int(sg["flags"]) >> k) & 1 and wrong != "skip_not_zeroed":
            continue
        b, c = int(sg["item_begin"]), items_of(int(sg["numel"]))
        if wrong == "neighbours_folded" and b + c < len(parts):
            c += 1
        if wrong == "last_item_dropped":
            c = max(c - 1, 1) if int(sg["numel"]) % ITEM == 0 else int(sg["numel"]) // ITEM
        p = parts[b:b + c]
        rounds = (c + WAVE - 1) // WAVE
        v = np.zeros(max(rounds, 1) * WAVE)
        v[:c] = p["sumsq"]
        acc = np.zeros(WAVE)
        for r in range(rounds):
            acc = acc + v[r * WAVE:(r + 1) * WAVE]
        out[s]["sumsq"] = _lane_fold(acc)
        out[s]["absmax"] = p["absmax"].max() if len(p) else 0
        out[s]["nonfinite"] = min(int(p["nonfinite"].sum()), 2 ** 32 - 1)
        out[s]["zeros"] = min(int(p["zeros"].sum()), 2 ** 32 - 1)
    return out


def restate(bufs, segments, wrong=None):
    """one dyk_tensor_stats call, restated -> STAT[nseg][nbuf]"""
    segs, items = work_list(segments)
    out = np.zeros((len(segs), len(bufs)), STAT)
    for k, b in enumerate(bufs):
        out[:, k] = fold(partials(b, items, wrong), segs, k, wrong)
    return out


WRONG_KERNELS = ("tail_vector_whole", "padding_in_zeros", "inf_taken", "neighbours_folded", "last_item_dropped", "skip_not_zeroed")


# ------------------------------------------------------------------ the plain reference
def plain_reference(bufs, segments):
    """-> [nseg][nbuf] of dict(norm, sumsq, absmax, nonfinite, zeros) or None for a skipped pair: np.sum over the finite x*x in
    fp64 (numpy's pairwise sum), exact max and counts"""
    out = []
    for (off, numel, flags) in segments:
        row = []
        for k, b in enumerate(bufs):
            if (flags >> k) & 1:
                row.append(None)
                continue
            x = np.asarray(b[off:off + numel], np.float32)
            fin = np.abs(x) <= np.float32(F32_MAX)
            xd = x[fin].astype(np.float64)
            s = float(np.sum(xd * xd))
            row.append(dict(norm=math.sqrt(s), sumsq=s, absmax=float(np.abs(x[fin]).max()) if fin.any() else 0.0,
                            nonfinite=int(np.count_nonzero(~fin)), zeros=int(np.count_nonzero(x == 0))))
        out.append(row)
    return out


def exact_sumsq(x):
    """math.fsum of the finite squares: the correctly rounded exact sum (small inputs only)"""
    x = np.asarray(x, np.float32)
    xd = x[np.abs(x) <= np.float32(F32_MAX)].astype(np.float64)
    return math.fsum((xd * xd).tolist())


def deviations(rec, bufs, segments, ref=None):
    """what of STAT[nseg][nbuf] `rec` is outside the contract, against the plain reference: a list of strings, [] when all is
    well (exact absmax / counts, norm within norm_bound, skipped records all zeros)"""
    ref = plain_reference(bufs, segments) if ref is None else ref
    bad = []
    for s, (off, numel, flags) in enumerate(segments):
        for k in range(len(bufs)):
            r, want = rec[s, k], ref[s][k]
            tag = "segment %d (offset %d, numel %d) buffer %d" % (s, off, numel, k)
            if want is None:
                if r.tobytes() != bytes(STAT.itemsize):
                    bad.append("%s: a skipped record is not all zeros" % tag)
                continue
            for f in ("nonfinite", "zeros"):
                if int(r[f]) != want[f]:
                    bad.append("%s: %s %d, exact %d" % (tag, f, int(r[f]), want[f]))
            if np.float32(r["absmax"]).view(np.uint32) != np.float32(want["absmax"]).view(np.uint32):
                bad.append("%s: absmax %r, exact %r" % (tag, float(r["absmax"]), want["absmax"]))
            norm = math.sqrt(float(r["sumsq"])) if r["sumsq"] >= 0 else float("nan")
            if not abs(norm - want["norm"]) <= norm_bound(numel) * want["norm"]:
                bad.append("%s: norm %.17g, fp64 %.17g (bound %.3g relative)" % (tag, norm, want["norm"], norm_bound(numel)))
            elif want["norm"] <= F32_MAX and not abs(float(np.float32(norm)) - want["norm"]) <= 2.0 ** -23 * want["norm"]:
                # (several FLT_MAX in one tensor: the norm is past the fp32 range, only the fp64 check above applies)
                bad.append("%s: fp32 norm %.9g, fp64 %.17g" % (tag, np.float32(norm), want["norm"]))
            if int(r["_pad"]) != 0:
                bad.append("%s: padding word not 0" % tag)
    return bad


# ------------------------------------------------------------------ synthetic tables
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 4095, 4096, 4097, 3 * 4096 + 1)
SPECIALS = (np.inf, -np.inf, np.nan, -0.0, 1e-41, F32_MAX)      # 1e-41: an fp32 denormal


def layout(lengths=LENGTHS, style="store", lead=8):
    """[(offset, numel)]: `store` rounds every offset up to 64 elements (the parameter store), `packed` to 4 only; `mixed`
    alternates.  `lead` elements in front of the first segment stay padding -> (segments, total elements, a multiple of 4)"""
    off = lead
    segs = []
    for i, ln in enumerate(lengths):
        a = 64 if style == "store" or (style == "mixed" and i % 2 == 0) else 4
        off = (off + a - 1) // a * a
        segs.append((off, ln))
        off += ln
        if style == "packed" and i % 3 == 2:
            off += 4                         # now and then a whole padding vector between packed segments
    return segs, (off + 64 + 3) // 4 * 4


def fill(segs, total, seed, pad=np.nan, scale=1.0):
    """a buffer of `total` floats: normal data of varying magnitude inside the segments, `pad` everywhere else"""
    rng = np.random.default_rng(seed)
    buf = np.full(total, pad, np.float32)
    for i, (off, ln) in enumerate(segs):
        buf[off:off + ln] = (rng.standard_normal(ln) * scale * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
    return buf


def special_spots(off, numel):
    """first and last element of a segment and both sides of every item boundary inside it"""
    spots = {0, numel - 1}
    for b in range(ITEM, numel, ITEM):
        spots |= {b - 1, b}
    return [off + s for s in sorted(spots)]


def plant_specials(buf, segs, shift=0):
    """SPECIALS at the special spots of every segment, cycling; `shift` starts the cycle elsewhere (a buffer of its own)"""
    buf = buf.copy()
    i = shift
    for off, ln in segs:
        for pos in special_spots(off, ln):
            buf[pos] = SPECIALS[i % len(SPECIALS)]
            i += 1
    return buf


def kernel_case(style, nbuf, specials=False, skips=False, seed=0):
    """-> (bufs, segments): the lengths of LENGTHS in the given layout, NaN between the segments, different data per buffer"""
    segs, total = layout(style=style)
    bufs = [fill(segs, total, seed * 16 + k) for k in range(nbuf)]
    if specials:
        bufs = [plant_specials(b, segs, shift=k) for k, b in enumerate(bufs)]
    flags = [0] * len(segs)
    if skips:
        for i in range(len(segs)):
            flags[i] = (i * 5 + 3) % (1 << nbuf) if i % 2 else 0      # some (segment, buffer) pairs; odd segments only
        flags[-1] = (1 << nbuf) - 1                                   # and the longest one for every buffer
    return bufs, [(o, n, f) for (o, n), f in zip(segs, flags)]


def wrong_kernel_cases():
    """name of a wrong kernel -> (bufs, segments) of the case that must flag it"""
    cases = {}
    # tail vector counted whole: 5 elements, then finite non-zero padding in the rest of the second vector
    segs, total = layout((5, 64), "store")
    cases["tail_vector_whole"] = ([fill(segs, total, 1, pad=3.0)], [(o, n, 0) for o, n in segs])
    # padding counted into zeros: the store's own padding is 0.0
    cases["padding_in_zeros"] = ([fill(segs, total, 2, pad=0.0)], [(o, n, 0) for o, n in segs])
    # inf taken into absmax / sumsq
    b = fill(segs, total, 3)
    b[segs[1][0] + 7] = np.inf
    cases["inf_taken"] = ([b], [(o, n, 0) for o, n in segs])
    # neighbours folded together / last item dropped: more than one item per segment, one of them a multiple of the item
    segs2, total2 = layout((4097, 2 * 4096, 65), "mixed")
    cases["neighbours_folded"] = ([fill(segs2, total2, 4)], [(o, n, 0) for o, n in segs2])
    cases["last_item_dropped"] = ([fill(segs2, total2, 5)], [(o, n, 0) for o, n in segs2])
    # a skipped segment not zeroed
    cases["skip_not_zeroed"] = ([fill(segs2, total2, 6), fill(segs2, total2, 7)], [(o, n, 2 if i == 1 else 0) for i, (o, n) in enumerate(segs2)])
    return cases
