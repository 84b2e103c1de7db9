"""fp16 inference mode, host side (CPU): dtype selection, the dry-compiled fp16 eval plan against the bf16 one (same commands
and buffers, element type swapped, fp32 islands untouched), the refusal of fp16 training plans, and the host reference of the
saturating float -> fp16 store (csrc/dyk_common.h: f32_to_f16) against clamp -> torch.half."""
import ctypes
import os
import shutil
import struct
import subprocess
import warnings

import pytest
import torch

from helpers import C1, C3, C5, INC, MNV2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ties with even and odd neighbours, the denormal range 2^-24 .. 2^-14, below 2^-25, the saturation edge, inf, NaN
F16_EDGE_VALUES = (
    [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20,
     2048.0 + 1.0, 2048.0 + 3.0, -(2048.0 + 1.0), 0.1, -0.3, 1e-3, 3.14159]
    + [2.0 ** e for e in range(-24, -13)] + [-(2.0 ** -24), 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -30, 1.5 * 2.0 ** -15,
                                             2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26]
    + [2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 + 2.0 ** -40, 2.0 ** -26, 2.0 ** -30, 1e-20]
    + [65504.0, -65504.0, 65503.9, 65519.0, 65520.0, -65520.0, 65536.0, 1e6, -1e6, 3e38, float("inf"), -float("inf"), float("nan")])


def f16_reference_bits(x):
    """the store rule of the fp16 path: clamp to +-65504 (NaN kept), round to nearest even; bits as int64"""
    return x.clamp(-65504.0, 65504.0).half().view(torch.int16).to(torch.int64) & 0xffff


# ------------------------------------------------------------------------------------------------ 1. dtype selection
class _M:
    training = False


@pytest.mark.parametrize("name", ["fp16", "float16", "half", torch.float16])
def test_fp16_names_select_float16(name, monkeypatch):
    from dyk.engine import _compute_dtype
    monkeypatch.delenv("DYK_DTYPE", raising=False)
    m = _M()
    m.dyk_dtype = name
    assert _compute_dtype(m) is torch.float16
    with torch.autocast("cpu", dtype=torch.bfloat16):            # an explicit request wins inside an autocast region
        assert _compute_dtype(m) is torch.float16


def test_dyk_dtype_env_selects_float16(monkeypatch):
    from dyk.engine import _compute_dtype
    monkeypatch.setenv("DYK_DTYPE", "fp16")
    assert _compute_dtype(_M()) is torch.float16


def test_fp16_autocast_region_still_selects_bf16_and_warns_once(monkeypatch):
    from dyk import engine
    monkeypatch.delenv("DYK_DTYPE", raising=False)
    monkeypatch.setattr(engine._compute_dtype, "warned", False)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda dev: torch.float16, raising=False)
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert engine._compute_dtype(_M()) is torch.bfloat16
        assert engine._compute_dtype(_M()) is torch.bfloat16
    mine = [x for x in w if "dyk:" in str(x.message)]
    assert len(mine) == 1
    assert "dyk_dtype = 'fp16'" in str(mine[0].message)


def test_dtype_code():
    from dyk import lib as L, ops
    assert L.DYK_F16 == 3
    assert ops.dtype_code(torch.float16) == L.DYK_F16
    assert ops.dtype_code(torch.bfloat16) == L.DYK_BF16 and ops.dtype_code(torch.float32) == L.DYK_F32


# ------------------------------------------------------------------------------------------------ 2. dry plans
def _plan(name, dtype, training=False, B=2, H=64, W=96):
    from build_utils.parse_config import materialize_cfg
    from dyk.params import ParamStore
    from dyk.plan import compile_plan
    from models import YOLO
    torch.manual_seed(0)
    m = YOLO(materialize_cfg(name))
    st = ParamStore(m)
    st.adopt(torch.device("cpu"))
    return compile_plan(m, st, B, H, W, dtype, training, torch.device("cpu"), dry=True), st


def _int_fields(d):
    """every integer field of a descriptor (shapes, strides, flags, tune words ...) -- pointers differ between two stores"""
    out = {}
    for f in d._fields_:
        name, tp = f[0], f[1]
        if tp in (ctypes.c_int32, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float):
            out[name] = getattr(d, name)
    return out


@pytest.mark.parametrize("name", [C1, C3, C5, INC, MNV2])
def test_fp16_eval_plan_is_the_bf16_plan_with_the_element_type_swapped(name):
    from dyk import lib as L
    ph, _ = _plan(name, torch.float16)
    pb, _ = _plan(name, torch.bfloat16)
    assert ph.dtype is torch.float16 and pb.dtype is torch.bfloat16
    assert [op for op, _ in ph.fwd] == [op for op, _ in pb.fwd]
    assert not ph.bwd and not pb.bwd
    assert {k: a.size for k, a in ph.arenas.items()} == {k: a.size for k, a in pb.arenas.items()}
    n16 = n32 = 0
    for (op, dh), (_, db) in zip(ph.fwd, pb.fwd):
        assert type(dh) is type(db)
        if not hasattr(dh, "_fields_"):
            continue
        fh, fb = _int_fields(dh), _int_fields(db)
        if "dtype" in fb:
            if fb["dtype"] == L.DYK_BF16:
                assert fh["dtype"] == L.DYK_F16, (op, fh["dtype"])
                n16 += 1
            else:                                        # fp32 islands: unchanged
                assert fh["dtype"] == fb["dtype"] == L.DYK_F32, (op, fh["dtype"], fb["dtype"])
                n32 += 1
            fh.pop("dtype"), fb.pop("dtype")
        assert fh == fb, (op, {k: (fh[k], fb[k]) for k in fh if fh[k] != fb[k]})
    assert n16 > 20
    # tensors: same placement and element sizes (heads stay fp32)
    for th, tb in zip(ph.outs, pb.outs):
        assert (th is None) == (tb is None)
        if th is not None:
            assert (th.arena, th.off, th.B, th.H, th.W, th.C, th.ld, th.esize) == (tb.arena, tb.off, tb.B, tb.H, tb.W, tb.C, tb.ld, tb.esize)
    assert all(p.dtype is torch.float32 for p in ph.p_out) and ph.io.dtype is torch.float32


def test_fp16_training_plan_is_refused():
    with pytest.raises(NotImplementedError, match="inference"):
        _plan(C1, torch.float16, training=True)


def test_tune_candidates_are_the_bf16_set_and_keys_differ():
    from dyk import lib as L, plan as P
    ph, _ = _plan(C1, torch.float16)
    pb, _ = _plan(C1, torch.bfloat16)
    seen = 0
    for (op, dh), (_, db) in zip(ph.fwd, pb.fwd):
        if op != L.OP_CONV:
            continue
        assert dh.dtype != db.dtype or db.dtype == L.DYK_F32
        assert P._conv_candidates(dh) == P._conv_candidates(db)
        assert P._conv_split_candidates(dh) == P._conv_split_candidates(db)
        seen += 1
    assert seen > 10


# ------------------------------------------------------------------------------------------------ 3. host conversion
_PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "dyk_common.h"
int main() {
    unsigned u;
    while (scanf("%x", &u) == 1) {
        float f; memcpy(&f, &u, 4);
        const f16_t h = f32_to_f16(f);
        const float back = f16_to_f32(h);
        unsigned ub; memcpy(&ub, &back, 4);
        printf("%04x %08x\n", (unsigned)h.v, ub);
    }
    return 0;
}
"""


def test_host_f32_to_f16_matches_clamp_then_half(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "probe.hip"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-I", os.path.join(ROOT, "double-yolo-kaist_amd", "csrc"),
                           str(src), "-o", str(exe)])
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.tensor(F16_EDGE_VALUES, dtype=torch.float32), torch.randn(4096, generator=g),
                   torch.randn(2048, generator=g) * 1e-6, torch.randn(2048, generator=g) * 3e4])
    bits = x.view(torch.int32).tolist()
    out = subprocess.run([str(exe)], input="\n".join("%x" % (b & 0xffffffff) for b in bits), capture_output=True, text=True, check=True)
    rows = [l.split() for l in out.stdout.splitlines()]
    assert len(rows) == x.numel()
    got = torch.tensor([int(r[0], 16) for r in rows], dtype=torch.int64)
    ref = f16_reference_bits(x)
    nan = torch.isnan(x)
    assert torch.equal(got[~nan], ref[~nan]), [(float(v), hex(int(a)), hex(int(b))) for v, a, b in zip(x[~nan], got[~nan], ref[~nan]) if a != b][:8]
    assert all(((int(b) & 0x7c00) == 0x7c00 and (int(b) & 0x3ff)) for b in got[nan])         # NaN stays NaN
    # and back: every fp16 value is exact in fp32
    back = torch.tensor([struct.unpack("<f", struct.pack("<I", int(r[1], 16)))[0] for r in rows], dtype=torch.float32)
    refb = x.clamp(-65504.0, 65504.0).half().float()
    assert torch.equal(back[~nan].view(torch.int32), refb[~nan].view(torch.int32))
