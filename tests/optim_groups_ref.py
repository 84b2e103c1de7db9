"""fp64 reference and derived per-element bounds of the GROUPED fused optimizer steps (dyk_adam_step_groups /
dyk_sgd_step_groups, csrc/optim.hip): one mask byte per element selects a parameter group (0 = frozen, k = group k-1) with its
own lr / weight_decay and, for Adam, decoupled weight decay (torch.optim.AdamW).  Shared by tests/test_optim_groups_reference.py
(CPU) and tests/test_gpu_optim_groups.py; built on oracle/optim.py, which is used as it stands.

L2 groups.  The update is elementwise, so the grouped step IS oracle.optim.adam_step_ref / sgd_step_ref evaluated on the elements
of each group with that group's lr and weight_decay: the reference and its bound are composed slice by slice, exactly.

Decoupled Adam (flags bit 0).  The kernel evaluates, in fp32,

    q    = p * decay_mul                 decay_mul = fl32(1 - fl32(lr * weight_decay)), formed on the host       1 rounding
    Adam statements on q with wd = 0     (oracle/optim.py: g', m', v', den, d, p' = q - d)

With wd = 0 neither g' nor m', v', den, d depend on p, so the exact result is  P' = P0 - D  with  P0 = p * decay_mul  (fp64) and
the references / bounds of m' and v' are the oracle's unchanged.  For p':

    |q - P0|            <= u|P0| + eta                                   (one rounded product; u = 2^-24, eta = 2^-149)
    |p'_kernel - (q-D)| <= e_p(q)                                        (the oracle's bound of the Adam statements at p = q)
    (q - D) - (P0 - D)   = q - P0                                        (exactly: D does not depend on p)
    =>  |p'_kernel - P'| <= e_p(q) + u|P0| + eta

q is not known to the reference, but fl32(P0) is (the product of two fp32 values rounds to the same fp32 value from its fp64
product as from the exact one, except on a double rounding tie, where the two candidates are neighbours and e_p differs by
u * ulp -- second order), so the published bound is  HEADROOM * e_p(fl32(P0))  [= the oracle's bound evaluated at fl32(P0)]
+ HEADROOM * (u|P0| + eta).  An fp32 evaluation in the kernel's statement order sits at <= 0.5 of it
(tests/test_optim_groups_reference.py), and the wrong group's lr, decay on a no-decay group, L2 for decoupled and the reverse,
decay_mul from another group's lr, and decay_mul applied after the update each exceed it on most elements.

Frozen bytes (0, or a byte above the group count): p, m, v pass through with bound 0."""
import numpy as np

from oracle.optim import ETA, HEADROOM, U, adam_step_ref, sgd_step_ref

f32 = np.float32
MAX_GROUPS = 8
DECOUPLED = 1


def decay_mul(lr, weight_decay):
    """fl32(1 - fl32(lr * weight_decay)) -- what DykOptimGroups carries for a decoupled group"""
    return f32(f32(1) - f32(lr) * f32(weight_decay))


def table(groups):
    """[(lr, weight_decay, decay_mul, flags)] with fp32 values held in Python floats, from dicts(lr, weight_decay[, decoupled])"""
    out = []
    for g in groups:
        lr, wd = f32(g["lr"]), f32(g["weight_decay"])
        out.append((float(lr), float(wd), float(decay_mul(lr, wd)), DECOUPLED if g.get("decoupled") else 0))
    return out


def adamw_formula(P, G, M, V, *, lr, weight_decay, beta1, beta2, eps, step):
    """-> (P', M', V'): the statements of the decoupled branch of grouped_step_ref with every scalar in double (no fp32
    decay_mul, bc1, bc2_sqrt, step_size, and grad_scale 1): what torch.optim.AdamW computes in float64"""
    P0 = P * (1.0 - lr * weight_decay)
    M1 = beta1 * M + (1.0 - beta1) * G
    V1 = beta2 * V + (1.0 - beta2) * G * G
    den = np.sqrt(V1) / np.sqrt(1.0 - beta2 ** step) + eps
    return P0 - (lr / (1.0 - beta1 ** step)) * (M1 / den), M1, V1


def interleaved_map(n, ngroups, frozen_every=5):
    """a group map over n elements in 64-element entries: entry e belongs to group e % ngroups, every `frozen_every`-th entry
    is frozen -- a group change (or a frozen entry) at every 64-element boundary"""
    e = np.arange(n) // 64
    gmap = (e % ngroups + 1).astype(np.uint8)
    if frozen_every:
        gmap[e % frozen_every == frozen_every - 1] = 0
    return gmap


def grouped_step_ref(kind, p, g, m, v, gmap, groups, *, beta1, beta2=0.0, eps=0.0, grad_scale=1.0, step=1):
    """-> (p', m', v', bound_p, bound_m, bound_v) float64 arrays (v', bound_v None for SGD without v).  gmap: one byte per
    element; groups: dicts(lr, weight_decay[, decoupled]).  Bytes 0 and bytes above len(groups) are frozen."""
    assert 1 <= len(groups) <= MAX_GROUPS
    p, g, m = (np.asarray(a, np.float32) for a in (p, g, m))
    v = None if v is None else np.asarray(v, np.float32)
    gmap = np.asarray(gmap, np.uint8)
    out = [p.astype(np.float64), m.astype(np.float64), None if v is None else v.astype(np.float64)]
    bounds = [np.zeros(p.size), np.zeros(p.size), None if v is None else np.zeros(p.size)]
    for k, (lr, wd, dm, flags) in enumerate(table(groups), 1):
        idx = np.flatnonzero(gmap == k)
        if idx.size == 0:
            continue
        ps, gs_, ms = p[idx], g[idx], m[idx]
        vs = None if v is None else v[idx]
        if kind == "sgd":
            if flags & DECOUPLED:
                raise ValueError("decoupled weight decay is not defined for the SGD step")
            r = sgd_step_ref(ps, gs_, ms, vs, None, lr=lr, beta1=beta1, weight_decay=wd, grad_scale=grad_scale, step=step)
        elif flags & DECOUPLED:
            with np.errstate(all="ignore"):
                P0 = ps.astype(np.float64) * dm
                q = P0.astype(np.float32)
                r = list(adam_step_ref(q, gs_, ms, vs, None, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=0.0,
                                       grad_scale=grad_scale, step=step))
                r[0] = r[0] + (P0 - q.astype(np.float64))                       # P0 - D
                r[3] = r[3] + HEADROOM * (U * np.abs(P0) + ETA)
        else:
            r = adam_step_ref(ps, gs_, ms, vs, None, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=wd,
                              grad_scale=grad_scale, step=step)
        for j in range(3):
            if out[j] is not None and r[j] is not None and not (kind == "sgd" and j == 2):
                out[j][idx] = r[j]
                bounds[j][idx] = r[3 + j]
    return out[0], out[1], out[2], bounds[0], bounds[1], bounds[2]
