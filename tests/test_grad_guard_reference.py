"""The arithmetic of the gradient guard (csrc/optim_guard.hip) restated in numpy (tests/grad_guard_ref.py) and checked on the
CPU: the reduction order against a plain fp64 norm, the fp32 clip coefficient, the record's state machine against
oracle.optim.adam_constants, the ctypes layouts of the two new structures against the C compiler's, and the keyword handling of
the fused optimizers that needs no GPU.  tests/test_gpu_grad_guard.py holds the kernels to the same restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import grad_guard_ref as R
from oracle.optim import adam_constants, input_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** -23


def _g(n, seed=1):
    return input_family(n, seed)[1]


@pytest.mark.parametrize("n,masked", [(4, False), (1028, False), (65540, True), (R.first_full_n(), False)])
def test_reduction_order_against_a_plain_fp64_norm(n, masked):
    g = _g(n, n % 97)
    mask = R.entry_mask(n) if masked else None
    gs = 1 / 8
    ref, _ = R.plain_reference(g, mask, gs)
    rec = R.stats(R.new_record(), g, mask, grad_scale=gs)
    assert ref > 0 and rec["nonfinite"] == 0 and rec["skip"] == 0 and rec["applied"] == 1
    assert abs(float(rec["norm"]) - ref) <= BOUND * ref
    # the fp64 sum itself sits far inside its bound (n * 2^-53, relative)
    assert abs(rec["sumsq"] - ref * ref) <= n * 2.0 ** -53 * ref * ref + 4 * 2.0 ** -53 * ref * ref
    assert R.grid_blocks(n) == {4: 1, 1028: 2, 65540: 65, R.first_full_n(): 1024}[n]
    if masked:
        full, _ = R.plain_reference(g, None, gs)
        assert full > ref                                     # the frozen entries do carry gradient
    if n == R.first_full_n():
        T = R.MAX_BLOCKS * R.BLOCK
        assert n // 4 == 2 * T + 1 and R.grid_blocks(n - 4) == R.MAX_BLOCKS


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
def test_non_finite_values_are_counted_where_live_and_only_there(value):
    n = 65540
    g = _g(n, 5)
    mask = R.entry_mask(n)
    live = np.flatnonzero(mask)
    frozen = np.flatnonzero(mask == 0)
    a = g.copy()
    a[[live[0], live[-1], live[len(live) // 2]]] = value
    rec = R.stats(R.new_record(), a, mask, skip_nonfinite=True, max_norm=1.0)
    assert rec["nonfinite"] == 3 and rec["skip"] == 1 and rec["applied"] == 0 and rec["skipped"] == 1
    assert not np.isfinite(rec["norm"])
    b = g.copy()
    b[[frozen[0], frozen[-1], frozen[len(frozen) // 2]]] = value
    rec = R.stats(R.new_record(), b, mask, skip_nonfinite=True)
    assert rec["nonfinite"] == 0 and rec["skip"] == 0 and np.isfinite(rec["norm"])
    assert rec["norm"] == R.stats(R.new_record(), g, mask)["norm"]
    # a finite gradient whose SCALED value overflows is non-finite for the update, and is counted
    c = g.copy()
    c[live[1]] = np.float32(3e38)
    assert R.stats(R.new_record(), c, mask, grad_scale=2.0)["nonfinite"] == 1
    assert R.stats(R.new_record(), c, mask, grad_scale=1.0)["nonfinite"] == 0


def test_clip_coefficient_cases():
    f = np.float32
    assert R.clip_coef(f(3.0), 0.0) == 1 and R.clip_coef(f(3.0), -1.0) == 1                  # off
    c = R.clip_coef(f(4.0), 2.0)
    assert c == f(2.0) / (f(4.0) + f(1e-6)) and 0.49 < c < 0.5                                # below 1
    assert R.clip_coef(f(1.0), 2.0) == 1                                                      # above 1: clamped
    assert np.isnan(R.clip_coef(f(np.nan), 2.0))                                              # NaN stays NaN (torch, too)
    assert R.clip_coef(f(np.inf), 2.0) == 0
    import torch
    for norm in (4.0, 1.0, float("nan"), float("inf")):
        want = torch.clamp(torch.tensor(2.0) / (torch.tensor(norm) + 1e-6), max=1.0).numpy()   # clip_grad_norm_'s own lines
        assert np.array_equal(np.float32(R.clip_coef(f(norm), 2.0)), want, equal_nan=True)


def test_the_gpu_tests_clip_choices_stay_away_from_the_coef_1_edge():
    """tests/test_gpu_grad_guard.py clips at 0.5 and 2 times the fp64 norm: the coefficient is then 0.5 / 1 with a margin that
    no rounding of the norm (2^-23 relative) can cross"""
    n = 65540
    g, mask = _g(n, 5), R.entry_mask(n)
    ref, _ = R.plain_reference(g, mask)
    for k in (1 - BOUND, 1 + BOUND):
        assert 0.49 < R.clip_coef(np.float32(ref * k), 0.5 * ref) < 0.51
        assert R.clip_coef(np.float32(ref * k), 2 * ref) == 1
        assert 2 * ref / (ref * k + 1e-6) > 1.9


def test_record_state_machine_over_clean_and_poisoned_steps():
    b1, b2 = 0.937, 0.999
    n = 1028
    clean, poisoned = _g(n, 9), _g(n, 9)
    poisoned[77] = np.inf
    script = [0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0]                  # 1 = a poisoned step (the first one included)
    rec = R.new_record()
    applied = skipped = 0
    for bad in script:
        before = dict(rec)
        rec = R.stats(rec, poisoned if bad else clean, None, max_norm=1.0, beta1=b1, beta2=b2, skip_nonfinite=True)
        applied, skipped = applied + (not bad), skipped + bad
        assert (rec["applied"], rec["skipped"], rec["skip"]) == (applied, skipped, bad)
        if bad:
            assert rec["bc1"] == before["bc1"] and rec["bc2_sqrt"] == before["bc2_sqrt"]
        else:
            _, _, bc1, bc2_sqrt, _ = adam_constants(b1, b2, 1e-3, applied)
            assert float(rec["bc1"]) == bc1 and float(rec["bc2_sqrt"]) == bc2_sqrt
    assert applied == 7 and skipped == 4
    # without skip_nonfinite a poisoned step is applied (and counted as such)
    rec = R.stats(R.new_record(), poisoned, None, beta1=b1, beta2=b2)
    assert (rec["applied"], rec["skipped"], rec["skip"], rec["nonfinite"]) == (1, 0, 0, 1)
    # SGD passes beta = 0: the corrections are 1
    rec = R.stats(R.new_record(), clean, None)
    assert rec["bc1"] == 1 and rec["bc2_sqrt"] == 1


NEW_STRUCTS = ["DykGradGuardRec", "DykGradStatsDesc"]


def test_new_struct_layouts_match_the_c_compiler(tmp_path):
    """the method of tests/test_abi.py, for every field of the two new structures"""
    from dyk import lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){"]
    for s in NEW_STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(lib, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for s in NEW_STRUCTS:
        cls = getattr(lib, s)
        assert int(out[s]) == ctypes.sizeof(cls), s
        for name, _ in cls._fields_:
            assert int(out["%s.%s" % (s, name)]) == getattr(cls, name).offset, (s, name)
    assert ctypes.sizeof(lib.DykGradGuardRec) == 40 and lib.DykGradGuardRec.applied.offset == 4 * 6
    assert lib.DykGradGuardRec.norm.offset == 8            # dyk.optim.clip_grad_norm_ returns a view of these four bytes


def test_entry_points_and_workspace_size_without_a_gpu():
    from dyk import lib
    h = lib.load()
    for n in (4, 1028, 65540, R.first_full_n(), 116_000_000):
        assert h.dyk_grad_stats_ws_bytes(n) == 16 * R.grid_blocks(n)
    assert h.dyk_grad_stats_ws_bytes(6) == 0 and h.dyk_grad_stats_ws_bytes(0) == 0
    assert h.dyk_grad_stats(None, None) == -1
    assert h.dyk_grad_stats(ctypes.byref(lib.DykGradStatsDesc()), None) == -1
    d = lib.DykOptimDesc()
    assert h.dyk_adam_step_guarded(ctypes.byref(d), None, None) == -1
    assert h.dyk_sgd_step_guarded(None, None, None) == -1
    assert h.dyk_grad_scale_by_rec(None, None, 4, None, None) == -1


def test_fused_optimizer_keywords_without_a_gpu():
    from build_utils.parse_config import materialize_cfg
    from dyk import optim
    from models import YOLO
    m = YOLO(materialize_cfg("kaist_yolov3"))
    for Opt in (optim.FusedAdam, optim.FusedSGD):
        o = Opt(m)
        assert not o._guarded and o._rec is None and o.max_grad_norm is None and o.skip_nonfinite is False
        assert o.grad_stats() is None and o.grad_stats(wait=True) is None
        o = Opt(m, max_grad_norm=10)
        assert o._guarded and o.max_grad_norm == 10.0 and not o.skip_nonfinite and o._rec is None
        o = Opt(m, skip_nonfinite=True)
        assert o._guarded and o.max_grad_norm is None and o._rec is None and o.grad_stats() is None
        for bad in (0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                Opt(m, max_grad_norm=bad)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(m, 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(m, 1.0, norm_type=float("inf"))
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(m, 0.0)
