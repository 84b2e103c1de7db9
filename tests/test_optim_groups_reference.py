"""tests/optim_groups_ref.py, the fp64 reference of the grouped fused optimizer steps and its per-element bound, and the host
side of parameter groups in dyk/optim.py (no GPU):
  * an fp32 evaluation in the kernel's statement order stays at <= 0.5 of every bound, on three (Adam: four) groups interleaved
    entry by entry with frozen entries in between;
  * the bound is not vacuous: six ways of confusing the groups each exceed it on more than half of the affected group;
  * the decoupled reference is torch.optim.AdamW in float64;
  * group_map(), the argument checks of the constructors and yolo_param_groups() on every detector cfg.
tests/test_gpu_optim_groups.py holds the HIP kernels to the same reference and bound."""
import numpy as np
import pytest
import torch

import optim_groups_ref as R
from oracle.optim import input_family
from test_optim_reference import _h32, _ratio, adam_emulation, sgd_emulation

f32 = np.float32
N = 64 * 50 * 16                    # 800 entries of 64 elements: 160 frozen, 160 per group (Adam, four groups)
L2 = [dict(lr=1e-3, weight_decay=5e-4), dict(lr=1e-3, weight_decay=0.0), dict(lr=2e-3, weight_decay=0.0)]
ADAMW = dict(lr=1e-3, weight_decay=1e-2, decoupled=True)
SHARED = dict(beta1=0.937, beta2=0.999, eps=1e-8)


def groups_of(kind):
    return L2 + [ADAMW] if kind == "adam" else L2


# ------------------------------------------------------------------ fp32 emulation of the grouped kernels
def emulate(kind, p, g, m, v, gmap, groups, *, beta1, beta2=0.0, eps=0.0, grad_scale=1.0, step=1, table=None, late_decay=False):
    """numpy float32, one rounding per operation, in the statement order of adam_vec / sgd_vec (csrc/optim.hip).  `table` replaces
    optim_groups_ref.table(groups) (the mutants hand in a confused one); late_decay applies decay_mul after the update."""
    p1, m1, v1 = p.copy(), m.copy(), v.copy()
    for k, (lr, wd, dm, flags) in enumerate(R.table(groups) if table is None else table, 1):
        idx = np.flatnonzero(gmap == k)
        ps, gs_, ms, vs = p[idx], g[idx], m[idx], v[idx]
        if kind == "sgd":
            p1[idx], m1[idx] = sgd_emulation(ps, gs_, ms, lr=lr, beta1=beta1, weight_decay=wd, grad_scale=grad_scale, step=step)
            continue
        dec = bool(flags & R.DECOUPLED)
        with np.errstate(all="ignore"):
            q = ps * f32(dm) if dec and not late_decay else ps
            a = adam_emulation(q, gs_, ms, vs, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=0.0 if dec else wd,
                               grad_scale=grad_scale, step=step)
            p1[idx], m1[idx], v1[idx] = (a[0] * f32(dm) if dec and late_decay else a[0]), a[1], a[2]
    return p1, m1, v1


def _case(kind, step, grad_scale, seed=0, n=N):
    h = dict(_h32(**SHARED), grad_scale=float(f32(grad_scale)), step=step)
    if kind == "sgd":
        h = dict(beta1=h["beta1"], grad_scale=h["grad_scale"], step=step)
    groups = groups_of(kind)
    p, g, m, v = input_family(n, seed, kind, h["beta1"], h["grad_scale"])
    return h, groups, (p, g, m, v), R.interleaved_map(n, len(groups))


@pytest.mark.parametrize("grad_scale", [1.0, 1 / 65536])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fp32_emulation_has_twofold_headroom(kind, grad_scale):
    worst = {}
    for step in (1, 2, 1000):
        h, groups, (p, g, m, v), gmap = _case(kind, step, grad_scale)
        ref = R.grouped_step_ref(kind, p, g, m, v, gmap, groups, **h)
        assert all(np.isfinite(r).all() for r in ref), "the family holds no non-finite element"
        got = emulate(kind, p, g, m, v, gmap, groups, **h)
        worst[step] = tuple(round(_ratio(a, r, b), 3) for a, r, b in zip(got, ref[:3], ref[3:]))
        frozen = gmap == 0
        assert frozen.sum() == N // 5
        for a, old, b in zip(ref[:3], (p, m, v), ref[3:]):
            assert np.array_equal(a[frozen], old[frozen].astype(np.float64)) and not b[frozen].any()
        assert np.all(ref[3][~frozen] > 0) and np.all(ref[4][~frozen] > 0)
    print("%s gs %g: grouped emulation / bound (p, m, v) per step: %s" % (kind, grad_scale, worst))
    assert max(max(w) for w in worst.values()) <= 0.5, worst


def test_l2_groups_are_the_oracle_slice_by_slice():
    from oracle.optim import adam_step_ref
    h, groups, (p, g, m, v), gmap = _case("adam", 2, 1.0, n=64 * 20)
    ref = R.grouped_step_ref("adam", p, g, m, v, gmap, groups, **h)
    whole = adam_step_ref(p, g, m, v, (gmap == 3), lr=2e-3, weight_decay=0.0, **h)
    sel = gmap == 3
    for a, b in zip(ref, whole):
        assert np.array_equal(a[sel], b[sel])
    # a byte above the group count is frozen
    part = R.grouped_step_ref("adam", p, g, m, v, gmap, groups[:2], **h)
    assert np.array_equal(part[0][gmap >= 3], p[gmap >= 3].astype(np.float64)) and not part[3][gmap >= 3].any()
    assert np.array_equal(part[0][gmap == 2], ref[0][gmap == 2])
    with pytest.raises(ValueError):
        R.grouped_step_ref("sgd", p, g, m, v, gmap, groups, beta1=0.937)


# ------------------------------------------------------------------ the bound tells the groups apart
def _beyond(got, ref, sel):
    """share of the elements of `sel` where p, m or v leaves its bound"""
    out = np.zeros(int(sel.sum()), bool)
    for a, r, b in zip(got, ref[:3], ref[3:]):
        out |= np.abs(a[sel].astype(np.float64) - r[sel]) > b[sel]
    return float(out.mean())


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_bound_catches_confused_groups(step):
    """groups 1..4 = L2 wd 5e-4 | no decay | no decay, lr 2e-3 | decoupled wd 1e-2.  Every mutant is an fp32 evaluation with one
    record of the table confused; the share is taken over the elements of the group that the confusion hits (an element counts when
    p, m or v leaves its bound -- the GPU test holds all three)."""
    h, groups, (p, g, m, v), gmap = _case("adam", step, 1.0)
    ref = R.grouped_step_ref("adam", p, g, m, v, gmap, groups, **h)
    t = R.table(groups)
    lr, wd, dm, fl = range(4)

    def swap(k, **kw):
        rec = list(t[k])
        for name, val in kw.items():
            rec[dict(lr=lr, wd=wd, dm=dm, fl=fl)[name]] = val
        return t[:k] + [tuple(rec)] + t[k + 1:]

    mutants = {
        "lr of the neighbouring group (2 takes 3's)": (2, dict(table=swap(1, lr=t[2][lr]))),
        "lr of the neighbouring group (3 takes 2's)": (3, dict(table=swap(2, lr=t[1][lr]))),
        "decay on the no-decay group": (2, dict(table=swap(1, wd=t[0][wd]))),
        "L2 where decoupled was asked for": (4, dict(table=swap(3, fl=0))),
        "decoupled where L2 was asked for": (1, dict(table=swap(0, fl=R.DECOUPLED))),
        "decay_mul from another group's lr": (4, dict(table=swap(3, dm=float(R.decay_mul(t[2][lr], t[3][wd]))))),
        "decay_mul applied after the update": (4, dict(late_decay=True)),
    }
    assert _beyond(emulate("adam", p, g, m, v, gmap, groups, **h), ref, gmap > 0) == 0.0
    share = {}
    for name, (k, kw) in mutants.items():
        got = emulate("adam", p, g, m, v, gmap, groups, **h, **kw)
        share[name] = round(_beyond(got, ref, gmap == k), 3)
        others = (gmap > 0) & (gmap != k)
        assert _beyond(got, ref, others) == 0.0, name
    print("step %d: share of the affected group beyond the bound: %s" % (step, share))
    assert min(share.values()) > 0.5, share


@pytest.mark.parametrize("step", [2, 1000])
def test_sgd_bound_catches_confused_groups(step):
    h, groups, (p, g, m, v), gmap = _case("sgd", step, 1.0)
    ref = R.grouped_step_ref("sgd", p, g, m, v, gmap, groups, **h)
    t = R.table(groups)
    share = {}
    for name, k, tab in (("lr of the neighbouring group", 3, t[:2] + [t[1]]), ("decay on the no-decay group", 2, [t[0], t[0], t[2]])):
        got = emulate("sgd", p, g, m, v, gmap, groups, **h, table=tab)
        sel = gmap == k
        share[name] = float(np.mean(np.abs(got[0][sel].astype(np.float64) - ref[0][sel]) > ref[3][sel]))
    print("sgd step %d: share of the affected group beyond bound_p: %s" % (step, share))
    assert min(share.values()) > 0.5, share


# ------------------------------------------------------------------ the decoupled reference is torch.optim.AdamW
def test_adamw_reference_is_torch_adamw_in_float64_over_five_steps():
    """optim_groups_ref.adamw_formula -- the statements of the decoupled branch with every scalar in double -- against
    torch.optim.AdamW(foreach=False) in float64: 1e-12 relative after each of five steps with a different gradient each.
    (grouped_step_ref itself carries decay_mul, bc1, bc2_sqrt and step_size rounded to fp32, as the kernel gets them: the next
    test shows that this is all that separates it from the formula.)"""
    n = 4096
    lr, wd, b1, b2, eps = (float(f32(x)) for x in (1e-3, 1e-2, 0.937, 0.999, 1e-8))
    rng = np.random.default_rng(11)
    P = rng.standard_normal(n) * 0.1
    M, V = np.zeros(n), np.zeros(n)
    tp = torch.tensor(P, dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for step in range(1, 6):
        G = rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1)
        before = np.abs(P)
        P, M, V = R.adamw_formula(P, G, M, V, lr=lr, weight_decay=wd, beta1=b1, beta2=b2, eps=eps, step=step)
        tp.grad = torch.tensor(G, dtype=torch.float64)
        opt.step()
        got = tp.detach().numpy()
        assert np.all(np.abs(P - got) <= 1e-12 * np.maximum(np.abs(got), before)), step
        s = opt.state[tp]
        assert np.allclose(M, s["exp_avg"].numpy(), rtol=1e-12, atol=0) and np.allclose(V, s["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert float(s["step"]) == 5.0 and np.abs(got - tp.detach().numpy()).max() == 0


def test_decoupled_reference_is_that_formula_up_to_the_fp32_scalars():
    """grouped_step_ref's decoupled branch against adamw_formula on the family's fp32 inputs: decay_mul is rounded to fp32
    (<= 2^-25 of p), step_size, bc1, bc2_sqrt likewise (<= 1e-6 of the update, as in tests/test_optim_reference.py)"""
    h, _, (p, g, m, v), _ = _case("adam", 3, 1.0, n=4096)
    ref = R.grouped_step_ref("adam", p, g, m, v, np.ones(4096, np.uint8), [ADAMW], **h)
    lr, wd = float(f32(ADAMW["lr"])), float(f32(ADAMW["weight_decay"]))
    P, G, M, V = (a.astype(np.float64) for a in (p, g, m, v))
    want = R.adamw_formula(P, G, M, V, lr=lr, weight_decay=wd, beta1=h["beta1"], beta2=h["beta2"], eps=h["eps"], step=3)
    upd = np.abs(want[0] - P * (1.0 - lr * wd))
    assert upd.max() > 0
    assert np.all(np.abs(ref[0] - want[0]) <= 1e-6 * upd + 2.0 ** -24 * np.abs(P))
    assert np.allclose(ref[1], want[1], rtol=1e-13, atol=1e-300) and np.allclose(ref[2], want[2], rtol=1e-13, atol=1e-300)


# ------------------------------------------------------------------ group_map
class _P:
    def __init__(self, requires_grad=True):
        self.requires_grad = requires_grad


def test_group_map_marks_entries_and_leaves_padding_and_frozen_entries_zero():
    from dyk.optim import group_map
    ps = [_P(), _P(), _P(False), _P(), _P()]
    entries = [(0, 64, ps[0]), (64, 3, ps[1]), (128, 100, ps[2]), (256, 130, ps[3]), (448, 1, ps[4])]
    groups = [dict(params=[ps[0], ps[3]]), dict(params=[ps[1], ps[2]]), dict(params=[ps[4]])]
    gm = group_map(entries, groups, 512)
    assert gm.dtype == np.uint8 and gm.shape == (512,)
    want = np.zeros(512, np.uint8)
    want[0:64], want[64:67], want[256:386], want[448] = 1, 2, 1, 3
    assert np.array_equal(gm, want)                                  # ps[2] is frozen: 0 although group 2 names it
    # every 16-byte vector that holds an element of a live entry reads as a 32-bit word whose low byte is the group, and every
    # vector that lies inside the entry is one constant word (k, k, k, k)
    words = gm.view(np.uint32)
    for off, n, p in entries:
        k = int(want[off])
        assert np.all((words[off // 4:(off + n + 3) // 4] & 0xff) == k)
        assert np.all(words[off // 4:(off + n) // 4] == k * 0x01010101)
    with pytest.raises(ValueError, match="more than one"):
        group_map(entries, [dict(params=[ps[0]]), dict(params=[ps[0]])], 512)
    with pytest.raises(ValueError):
        group_map(entries, [dict(params=[p]) for p in ps] * 2, 512)
    with pytest.raises(ValueError):
        group_map(entries, [], 512)
    assert not group_map(entries, [dict(params=[])], 512).any()       # parameters of no group stay 0


# ------------------------------------------------------------------ constructors and yolo_param_groups on every detector cfg
def _yolo(name):
    from build_utils.parse_config import materialize_cfg
    from models import YOLO
    torch.manual_seed(0)
    return YOLO(materialize_cfg(name))


def test_constructor_rejects_groups_that_do_not_partition_the_trainable_parameters():
    from dyk.optim import FusedAdam, FusedAdamW, FusedSGD, yolo_param_groups
    m = _yolo("kaist_yolov3")
    names = dict((id(p), n) for n, p in m.named_parameters())
    groups = yolo_param_groups(m, 5e-4)
    opt = FusedAdam(m, lr=1e-3, param_groups=groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [5e-4, 0.0, 0.0] and all(g["lr"] == 1e-3 for g in opt.param_groups)
    assert opt._grouped() and not FusedAdam(m, lr=1e-3)._grouped() and FusedAdamW(m)._grouped()
    assert FusedAdamW(m).param_groups[0]["weight_decay"] == 1e-2 and FusedAdamW(m).param_groups[0]["decoupled_weight_decay"] is True
    missing = groups[0]["params"][3]
    with pytest.raises(ValueError, match=names[id(missing)].replace(".", r"\.") + " is in no parameter group"):
        FusedAdam(m, param_groups=[dict(groups[0], params=[p for p in groups[0]["params"] if p is not missing])] + groups[1:])
    dup = groups[1]["params"][0]
    with pytest.raises(ValueError, match=names[id(dup)].replace(".", r"\.") + " appears in more than one"):
        FusedSGD(m, param_groups=groups[:2] + [dict(groups[2], params=groups[2]["params"] + [dup])])
    with pytest.raises(ValueError, match="not a trainable parameter"):
        FusedAdam(m, param_groups=groups + [dict(params=[torch.nn.Parameter(torch.zeros(3))])])
    every = [p for g in groups for p in g["params"]]
    with pytest.raises(ValueError, match="1 to 8 parameter groups, got 9"):
        FusedAdam(m, param_groups=[dict(params=every[i::9]) for i in range(9)])
    assert len(FusedAdam(m, param_groups=[dict(params=every[i::8]) for i in range(8)]).param_groups) == 8
    with pytest.raises(ValueError, match="betas"):
        FusedAdam(m, betas=(0.937, 0.999), param_groups=[dict(groups[0], betas=(0.9, 0.999))] + groups[1:])
    FusedAdam(m, betas=(0.937, 0.999), param_groups=[dict(groups[0], betas=(0.937, 0.999))] + groups[1:])       # the shared value is fine
    with pytest.raises(ValueError, match="eps"):
        FusedAdam(m, param_groups=[dict(groups[0], eps=1e-6)] + groups[1:])
    with pytest.raises(ValueError, match="momentum"):
        FusedSGD(m, momentum=0.937, param_groups=[dict(groups[0], momentum=0.9)] + groups[1:])
    with pytest.raises(ValueError, match="nesterov"):
        FusedSGD(m, param_groups=[dict(groups[0], nesterov=False)] + groups[1:])
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        FusedSGD(m, param_groups=[dict(groups[0], decoupled_weight_decay=True)] + groups[1:])
    mixed = FusedAdam(m, param_groups=[dict(groups[0], decoupled_weight_decay=True, lr=5e-4)] + groups[1:])
    t = mixed._group_table()
    assert t.count == 3 and t.g[0].flags == 1 and t.g[1].flags == 0
    assert f32(t.g[0].decay_mul) == R.decay_mul(5e-4, 5e-4) and f32(t.g[0].lr) == f32(5e-4) and f32(t.g[1].lr) == f32(1e-3)


def _detector_cfgs():
    from test_all_cfgs import NAMES
    return NAMES


@pytest.mark.parametrize("name", _detector_cfgs())
def test_yolo_param_groups_partition_every_detector_cfg(name):
    import torch.nn as nn
    from build_utils.layers import WeightedFeatureFusion
    from dyk.optim import FusedSGD, group_map, yolo_param_groups
    m = _yolo(name)
    frozen = [p for i in range(3) for p in m.module_list[i].parameters()]
    for p in frozen:
        p.requires_grad_(False)
    groups = yolo_param_groups(m, 5e-4, bias_lr=0.1)
    assert len(groups) == 3 and groups[2]["lr"] == 0.1 and "lr" not in groups[0] and "lr" not in groups[1]
    assert [g["weight_decay"] for g in groups] == [5e-4, 0.0, 0.0]
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids)) and set(ids) == {id(p) for p in m.parameters() if p.requires_grad}
    assert not set(ids) & {id(p) for p in frozen}
    norm_or_bias = set()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            norm_or_bias |= {id(p) for p in mod.parameters(recurse=False)}
        elif isinstance(mod, WeightedFeatureFusion):
            norm_or_bias |= {id(p) for p in mod.parameters(recurse=False)}
        elif getattr(mod, "bias", None) is not None:
            norm_or_bias.add(id(mod.bias))
    assert not norm_or_bias & {id(p) for p in groups[0]["params"]}
    assert all(p.dim() >= 2 for p in groups[0]["params"]) and groups[0]["params"] and groups[1]["params"] and groups[2]["params"]
    assert {id(p) for p in groups[1]["params"]} | {id(p) for p in groups[2]["params"]} == norm_or_bias - {id(p) for p in frozen}
    opt = FusedSGD(m, lr=1e-2, momentum=0.937, param_groups=groups)     # ... and the constructor takes them
    st = m.engine.store
    gm = group_map(st.entries, opt.param_groups, st.total)
    for e in st.entries:
        want = 0 if not e.param.requires_grad else 1 + next(k for k, g in enumerate(groups) if any(e.param is p for p in g["params"]))
        assert np.all(gm[e.offset:e.offset + e.numel] == want) and not gm[e.offset + e.numel:e.offset + (e.numel + 63) // 64 * 64].any()


# ------------------------------------------------------------------ the ABI of the grouped entries (no GPU)
def test_group_table_layout_matches_the_c_compiler(tmp_path):
    import os
    import subprocess
    from dyk import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dyk_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %d %d\\n", sizeof(DykOptimGroup), sizeof(DykOptimGroups), offsetof(DykOptimGroups, g), '
                   'offsetof(DykOptimGroup, flags), DYK_OPT_MAX_GROUPS, DYK_OPT_GROUP_DECOUPLED);return 0;}')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [ctypes_sizeof(lib.DykOptimGroup), ctypes_sizeof(lib.DykOptimGroups), lib.DykOptimGroups.g.offset,
                   lib.DykOptimGroup.flags.offset, lib.OPT_MAX_GROUPS, lib.OPT_GROUP_DECOUPLED]
    assert lib.OPT_MAX_GROUPS == R.MAX_GROUPS == 8 and lib.OPT_GROUP_DECOUPLED == R.DECOUPLED


def ctypes_sizeof(cls):
    import ctypes
    return ctypes.sizeof(cls)


BAD = ["desc_null", "groups_null", "mask_null", "mask_misaligned", "count_0", "count_9", "wd_negative", "wd_nan", "lr_nan", "lr_inf",
       "unknown_flag", "step_zero", "rec_misaligned", "n_not_4", "p_null", "decoupled_sgd"]


@pytest.mark.parametrize("fn,bad", [(fn, bad) for fn in ("dyk_adam_step_groups", "dyk_sgd_step_groups") for bad in BAD
                                    if (fn, bad) != ("dyk_adam_step_groups", "decoupled_sgd")])    # valid for Adam: it would launch
def test_bad_arguments_are_rejected_before_any_launch(fn, bad):
    """no GPU here: a launch would fail with DYK_ERR_HIP (-2), not DYK_ERR_ARG (-1) / DYK_ERR_UNSUPPORTED (-3); the addresses are
    never dereferenced.  (tests/test_gpu_optim_groups.py repeats this on the device and checks that no buffer changes.)"""
    import ctypes
    from dyk import lib
    from test_optim_reference import _fake_desc
    call = getattr(lib.load(), fn)
    d = _fake_desc(step=2)
    t = lib.DykOptimGroups()
    t.count = 3
    for k, (lr, wd, dm, flags) in enumerate(R.table(L2)):
        t.g[k].lr, t.g[k].weight_decay, t.g[k].decay_mul, t.g[k].flags = lr, wd, dm, flags
    dref, tref, rec, want = ctypes.byref(d), ctypes.byref(t), None, -1
    if bad == "desc_null":
        dref = None
    elif bad == "groups_null":
        tref = None
    elif bad == "mask_null":
        d.mask = None
    elif bad == "mask_misaligned":
        d.mask += 2
    elif bad == "count_0":
        t.count = 0
    elif bad == "count_9":
        t.count = 9
    elif bad == "wd_negative":
        t.g[0].weight_decay = -5e-4
    elif bad == "wd_nan":
        t.g[1].weight_decay = float("nan")
    elif bad == "lr_nan":
        t.g[1].lr = float("nan")
    elif bad == "lr_inf":
        t.g[2].lr = float("-inf")
    elif bad == "unknown_flag":
        t.g[2].flags = 4
    elif bad == "step_zero":
        d.step = 0
    elif bad == "rec_misaligned":
        rec = ctypes.c_void_p(0x70004)
    elif bad == "n_not_4":
        d.n = 62
    elif bad == "p_null":
        d.p = None
    elif bad == "decoupled_sgd":
        t.g[0].flags = 1
        want = -3
    assert call(dref, tref, rec, None) == want
