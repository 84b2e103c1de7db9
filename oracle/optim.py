"""fp64 restatement of the fused optimizer steps (csrc/optim.hip: dyk_adam_step / dyk_sgd_step, the update rules of
torch.optim.Adam and torch.optim.SGD(nesterov=True, dampening=0) with L2 weight decay added to the gradient, reference
train.py:85-91) and a DERIVED per-element bound on what an fp32 evaluation of the same formula may differ by.

The hyper-parameters are taken as the descriptor carries them (fp32), and the scalar constants are formed as the kernel
forms them, so that the bound measures the per-element arithmetic only:

    1 - beta   = fl32(1) - fl32(beta)               (exact in fp32 for beta in [0.5, 1))
    bc1        = fl32(1 - beta1^step)               (formed in double)
    bc2_sqrt   = fl32(sqrt(1 - beta2^step))         (formed in double)
    step_size  = fl32(fl32(lr) / bc1)

How far these are from torch.optim's double-precision scalars is a separate check (tests/test_optim_reference.py).

Bound.  u = 2^-24 is the unit roundoff of fp32, eta = 2^-149 its smallest denormal (the absolute error of a result that
underflows, gradual or flushed to the next denormal; every stage carries one eta per rounded operation).  Each stage's error
is (number of rounded operations) x u x (magnitude of the TERMS of that stage, not of its result -- the bound has to survive
cancellation in b1*m + (1-b1)*g') plus the propagated error of its inputs to first order.  A contracted multiply-add (hipcc's
-ffp-contract=on) only removes roundings; division and sqrtf are correctly rounded in the library's build.

    Adam                                                          rounded operations
    g'   = g*gs + wd*p                                            2 products + 1 sum: at most 2u on each term
    m'   = b1*m + (1-b1)*g'                                       3 (two products, one sum)
    v'   = b2*v + ((1-b2)*g')*g'                                  4
    den  = sqrt(v')/bc2_sqrt + eps                                1 (sqrt) + 2
    d    = step_size * (m'/den)                                   2 (+1 for the second-order terms of the quotient)
    p'   = p - d                                                  1, on max(|p|, |p'|) <= |p| + |p'|

      e_g' = 2u(|g*gs| + |wd*p|)
      e_m  = (1-b1)*e_g' + 3u(|b1*m| + |(1-b1)*g'|)
      e_v  = (1-b2)*2|g'|*e_g' + 4u(|b2*v| + (1-b2)*g'^2)
      e_sq = |sqrt(v') - sqrt(v' +- e_v)| + u*sqrt(v')  with  |sqrt a - sqrt b| = |a-b| / (sqrt a + sqrt b) <= sqrt|a-b|
      e_den= e_sq/bc2_sqrt + 2u*den
      e_d  = step_size*(e_m/den + |m'|/den^2 * e_den) + 3u|d|
      e_p  = e_d + u(|p| + |p'|)

    SGD-Nesterov                                                  rounded operations
    g'   = g*gs + wd*p                                            as above
    m'   = g' (first step)  |  mom*m + g'                         0 | 2
    s    = g' + mom*m'                                            2
    p'   = p - lr*s                                               1 product, 1 difference

      e_m  = e_g' + 2u(|mom*m| + |g'|)          (first step: e_g')
      e_s  = e_g' + mom*e_m + 2u(|g'| + |mom*m'|)
      e_p  = lr*e_s + u|lr*s| + u(|p| + |p'|)

These e_* are worst cases that the fp32 arithmetic attains to within a few per cent on 2^20 elements (two-operation stages such
as SGD's m' reach 0.99 of them).  The published bounds are HEADROOM x e_*: a kernel with the statement order of optim.hip then
sits at <= 0.5 of every bound (tests/test_optim_reference.py asserts it on the input family below), which leaves room for another
order of the same operations (the compiler's contraction choices) and none for a wrong formula: the same test shows that swapped
betas, bc2 for sqrt(bc2), eps inside the root, decoupled weight decay, plain momentum and a misplaced first-step rule each
exceed the bound on most elements.

Frozen elements (mask byte 0) keep p, m, v; their bounds are 0 (bit equality).
Non-finite inputs give non-finite references and bounds, element by element as in torch.optim; callers compare those by class.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149
HEADROOM = 2.0


def _f32(x):
    return float(np.float32(x))


def adam_constants(beta1, beta2, lr, step):
    """(1-beta1, 1-beta2, bc1, bc2_sqrt, step_size) as dyk_adam_step forms them, returned as Python floats holding fp32 values"""
    b1, b2 = np.float32(beta1), np.float32(beta2)
    omb1, omb2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    bc1 = _f32(1.0 - float(b1) ** int(step))
    bc2_sqrt = _f32(np.sqrt(1.0 - float(b2) ** int(step)))
    with np.errstate(divide="ignore"):
        step_size = float(np.float32(lr) / np.float32(bc1))
    return omb1, omb2, bc1, bc2_sqrt, step_size


def _prep(arrays, mask):
    out = [None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64) for a in arrays]
    live = None if mask is None else np.asarray(mask).astype(bool)
    return out, live


def _freeze(live, new, old, bounds):
    if live is None:
        return new, bounds
    return [np.where(live, a, b) for a, b in zip(new, old)], [np.where(live, e, 0.0) for e in bounds]


def adam_step_ref(p, g, m, v, mask=None, *, lr, beta1, beta2, eps, weight_decay, grad_scale, step):
    """-> (p', m', v', bound_p, bound_m, bound_v), float64 arrays.  p, g, m, v: fp32 arrays; mask: None or one byte per element
    (0 = frozen); hyper-parameters are rounded to fp32 first, as DykOptimDesc stores them."""
    if step <= 0:
        raise ValueError("step is 1-based")
    (P, G, M, V), live = _prep((p, g, m, v), mask)
    lr, b1, b2, eps, wd, gs = (_f32(x) for x in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    omb1, omb2, bc1, bc2s, ss = adam_constants(b1, b2, lr, step)
    u, eta = U, ETA
    with np.errstate(all="ignore"):
        gr = G * gs + wd * P
        M1 = b1 * M + omb1 * gr
        V1 = b2 * V + omb2 * gr * gr
        root = np.sqrt(V1)
        den = root / bc2s + eps
        D = ss * (M1 / den)
        P1 = P - D
        e_gr = 2 * u * (np.abs(G * gs) + np.abs(wd * P)) + 3 * eta
        e_m = omb1 * e_gr + 3 * u * (np.abs(b1 * M) + np.abs(omb1 * gr)) + 3 * eta
        e_v = omb2 * 2 * np.abs(gr) * e_gr + 4 * u * (np.abs(b2 * V) + omb2 * gr * gr) + 4 * eta
        e_sq = np.where(V1 > e_v, e_v / (root + np.sqrt(np.maximum(V1 - e_v, 0.0))), np.sqrt(e_v)) + u * root + eta
        e_den = e_sq / bc2s + 2 * u * den + 2 * eta
        e_D = ss * (e_m / den + np.abs(M1) / den ** 2 * e_den) + 3 * u * np.abs(D) + 2 * eta
        e_p = e_D + u * (np.abs(P) + np.abs(P1)) + eta
    new, bounds = _freeze(live, [P1, M1, V1], [P, M, V], [HEADROOM * e_p, HEADROOM * e_m, HEADROOM * e_v])
    return tuple(new) + tuple(bounds)


def sgd_step_ref(p, g, m, v=None, mask=None, *, lr, beta1, weight_decay, grad_scale, step, beta2=0.0, eps=0.0):
    """SGD with Nesterov momentum `beta1`, dampening 0: -> (p', m', v', bound_p, bound_m, bound_v).  v is passed through (the
    kernel neither reads nor writes it; None stays None) with bound 0; beta2 / eps are accepted and unused, as in the descriptor."""
    if step <= 0:
        raise ValueError("step is 1-based")
    (P, G, M), live = _prep((p, g, m), mask)
    lr, mom, wd, gs = (_f32(x) for x in (lr, beta1, weight_decay, grad_scale))
    first = step == 1
    u, eta = U, ETA
    with np.errstate(all="ignore"):
        gr = G * gs + wd * P
        M1 = gr if first else mom * M + gr
        S = gr + mom * M1
        P1 = P - lr * S
        e_gr = 2 * u * (np.abs(G * gs) + np.abs(wd * P)) + 3 * eta
        e_m = e_gr if first else e_gr + 2 * u * (np.abs(mom * M) + np.abs(gr)) + 2 * eta
        e_s = e_gr + mom * e_m + 2 * u * (np.abs(gr) + np.abs(mom * M1)) + 2 * eta
        e_p = lr * e_s + u * np.abs(lr * S) + u * (np.abs(P) + np.abs(P1)) + 2 * eta
    (P1, M1), (b_p, b_m) = _freeze(live, [P1, M1], [P, M], [HEADROOM * e_p, HEADROOM * e_m])
    V = None if v is None else np.asarray(v, dtype=np.float32).astype(np.float64)
    return P1, M1, V, b_p, b_m, (None if v is None else np.zeros_like(V))


def input_family(n, seed, kind="adam", beta1=0.937, grad_scale=1.0):
    """The seeded inputs the optimizer tests share: fp32 arrays (p, g, m, v) of n elements.
      * normals times 10^k, k drawn per element: k in [-8, 1] for g, m and sqrt(v), k in [-4, 0] for p;
      * exact zeros at strides 7, 11, 13 in g, m, v;
      * a cancellation stripe (5::17): m such that the decayed moment cancels the new gradient term
        (Adam: b1*m = -(1-b1)*g*gs; SGD: mom*m = -g*gs);
      * a stripe of tiny gradients (3::19, g = 1e-25): g^2 underflows in fp32, Adam's denominator is eps alone."""
    f = np.float32
    rng = np.random.default_rng(seed)

    def mags(lo, hi):
        return (rng.standard_normal(n) * 10.0 ** rng.integers(lo, hi + 1, n)).astype(f)
    p, g, m = mags(-4, 0), mags(-8, 1), mags(-8, 1)
    v = (mags(-8, 1).astype(np.float64) ** 2).astype(f)
    g[::7] = 0
    m[::11] = 0
    v[::13] = 0
    b1, gs = float(f(beta1)), float(f(grad_scale))
    stripe = g[5::17].astype(np.float64) * gs
    m[5::17] = (-(1.0 - b1) / b1 * stripe if kind == "adam" else -stripe / b1).astype(f)
    g[3::19] = f(1e-25)
    return p, g, m, v
