"""numpy restatement of the gradient statistics of csrc/optim_guard.hip (dyk_grad_stats) -- the reduction ORDER of the partials
and finalize kernels, the fp32 clip coefficient and the record's state machine -- plus the plain fp64 reference the tests hold
the device to.  Shared by tests/test_grad_guard_reference.py (CPU) and the GPU tests; not an oracle of the reference project.

Order (include/dyk_hip.h): grid = min(ceil(n/4 / 256), 1024) blocks of 256 threads; thread t of the grid takes the 16-byte
vectors t, t + T, t + 2T, ... (T = threads of the grid) and adds x*x of their four elements in order, x = fl32(g * grad_scale);
64 lanes fold as l += l+32, l+16, ..., l+1; the four waves of a block add in order; the blocks add in index order.

Error of that order against the exact sum (what the 2^-23 bound of the tests rests on): every x*x is exact in fp64 (two 24-bit
significands), all terms are >= 0, and a term passes through at most  min(n - 1, ceil(n/4 / T) * 4 + 6 + 3 + 1024)  additions
that round (adding an exact zero does not), each with relative error <= 2^-53: |sumsq - exact| <= n * 2^-53 * exact in any
case and <= 1100 * 2^-53 * exact up to n = 2^24.  The root halves it; rounding the root to double and then to fp32 adds 2^-53
and 2^-24:  |norm - ref| <= (2^-24 + 2^-53 + n * 2^-54) * ref  <  2^-23 * ref  for n < 2^29."""
import numpy as np

BLOCK = 256
MAX_BLOCKS = 1024
WAVE = 64
F32_MAX = float(np.finfo(np.float32).max)


def grid_blocks(n):
    return min((n // 4 + BLOCK - 1) // BLOCK, MAX_BLOCKS)


def first_full_n():
    """the smallest n that gives every thread of the capped grid two vectors, plus a tail vector for thread 0"""
    return (MAX_BLOCKS * BLOCK * 2 + 1) * 4


def scaled(g, grad_scale):
    """x = fl32(g * grad_scale), the value the update consumes"""
    with np.errstate(all="ignore"):
        return np.asarray(g, np.float32) * np.float32(grad_scale)


def live_elements(n, mask):
    """which elements the kernel takes: all, or those of 16-byte vectors whose four mask bytes are not all 0"""
    if mask is None:
        return np.ones(n, bool)
    return np.repeat(np.asarray(mask, np.uint8).reshape(-1, 4).any(axis=1), 4)


def plain_reference(g, mask=None, grad_scale=1.0):
    """-> (norm, nonfinite): sqrt(sum(x*x)) in fp64 with numpy's own (pairwise) sum, and the exact count"""
    x = scaled(g, grad_scale).astype(np.float64)[live_elements(len(g), mask)]
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.sum(x * x))), int(np.count_nonzero(~(np.abs(x) <= F32_MAX)))


def partials(g, mask=None, grad_scale=1.0):
    """-> (sumsq[nb] float64, nonfinite[nb]) exactly as the partials kernel leaves them in its workspace"""
    n = len(g)
    assert n > 0 and n % 4 == 0
    nb = grid_blocks(n)
    T = nb * BLOCK
    x = scaled(g, grad_scale).astype(np.float64)
    live = live_elements(n, mask)
    with np.errstate(all="ignore"):
        sq = np.where(live, x * x, 0.0)                      # (acc + 0.0 == acc: a skipped vector leaves the sum alone)
    bad = (live & ~(np.abs(x) <= F32_MAX)).astype(np.int64)
    sweeps = (n // 4 + T - 1) // T
    pad = sweeps * T * 4 - n
    sq = np.concatenate([sq, np.zeros(pad)]).reshape(sweeps, T, 4)
    bad = np.concatenate([bad, np.zeros(pad, np.int64)]).reshape(sweeps, T, 4)
    acc = np.zeros(T)
    with np.errstate(all="ignore"):
        for k in range(sweeps):
            for j in range(4):
                acc = acc + sq[k, :, j]
        a = acc.reshape(nb, BLOCK // WAVE, WAVE).copy()
        off = WAVE // 2
        while off:
            a[..., :off] = a[..., :off] + a[..., off:2 * off]
            off //= 2
        waves = a[..., 0]
        block = waves[:, 0]
        for w in range(1, BLOCK // WAVE):
            block = block + waves[:, w]
    return block, bad.sum(axis=(0, 2)).reshape(nb, BLOCK).sum(axis=1)


def fold(block_sumsq, block_bad):
    """the finalize kernel's sum: block-index order, fp64; the count saturates at 2^32 - 1"""
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for v in block_sumsq:
            s = s + v
    return float(s), int(min(int(np.sum(block_bad)), 2 ** 32 - 1))


def clip_coef(norm, max_norm):
    """fp32: c = max_norm / (norm + 1e-6f); coef = max_norm > 0 ? (c > 1 ? 1 : c) : 1 -- a NaN norm gives a NaN coef"""
    f = np.float32
    with np.errstate(all="ignore"):
        c = f(max_norm) / (f(norm) + f(1e-6))
    if not f(max_norm) > 0:
        return f(1.0)
    return f(1.0) if c > 1 else c


def new_record():
    return dict(sumsq=0.0, norm=np.float32(0), coef=np.float32(0), nonfinite=0, skip=0, applied=0, skipped=0,
                bc1=np.float32(0), bc2_sqrt=np.float32(0))


def finalize(rec, sumsq, nonfinite, *, max_norm=0.0, beta1=0.0, beta2=0.0, skip_nonfinite=False):
    """the finalize lane: -> the record after one dyk_grad_stats call (a new dict)"""
    f = np.float32
    r = dict(rec)
    with np.errstate(all="ignore"):
        r["sumsq"] = float(sumsq)
        r["norm"] = f(np.sqrt(np.float64(sumsq)))
    r["coef"] = clip_coef(r["norm"], max_norm)
    r["nonfinite"] = int(nonfinite)
    r["skip"] = 1 if (skip_nonfinite and nonfinite > 0) else 0
    if not r["skip"]:
        t = r["applied"] = rec["applied"] + 1
        r["bc1"] = f(1.0 - float(f(beta1)) ** t)
        r["bc2_sqrt"] = f(np.sqrt(1.0 - float(f(beta2)) ** t))
    else:
        r["skipped"] = rec["skipped"] + 1
    return r


def stats(rec, g, mask=None, *, grad_scale=1.0, **kw):
    """one dyk_grad_stats call, restated"""
    s, c = fold(*partials(g, mask, grad_scale))
    return finalize(rec, s, c, **kw)


def entry_mask(n):
    """a trainable mask that freezes whole 64-element entries: the first, the last (with the ragged tail), three in the middle"""
    m = np.ones(n, np.uint8)
    m[:64] = 0
    m[(n - 1) // 64 * 64 - 64:] = 0
    mid = n // 128 * 64
    m[mid:mid + 192] = 0
    return m
