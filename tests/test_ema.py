"""ModelEMA (reference build_utils/torch_utils.py:77-126) without a GPU: public surface, decay ramp, the C ABI of
dyk_ema_update (layout, argument checks before any launch), YOLO deepcopy, and the refusals."""
import copy
import ctypes
import inspect
import math
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _yolo(name="kaist_dyolov3_add_sl"):
    from build_utils.parse_config import materialize_cfg
    from models import YOLO
    torch.manual_seed(0)
    return YOLO(materialize_cfg(name))


def test_model_ema_surface_matches_the_reference():
    from build_utils.torch_utils import ModelEMA
    sig = inspect.signature(ModelEMA.__init__)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("model", inspect.Parameter.empty), ("decay", 0.9999), ("device", "")]
    assert list(inspect.signature(ModelEMA.update).parameters) == ["self", "model"]
    assert list(inspect.signature(ModelEMA.update_attr).parameters) == ["self", "model"]


def test_decay_ramp_and_initial_state():
    from build_utils.torch_utils import ModelEMA
    m = _yolo()
    ema = ModelEMA(m)
    assert ema.updates == 0 and ema.device == "" and not ema.ema.training
    assert all(not p.requires_grad for p in ema.ema.parameters())
    assert all(p.requires_grad for p in m.parameters())
    for x in (1, 2, 10, 2000, 10 ** 6):
        assert ema.decay(x) == 0.9999 * (1 - math.exp(-x / 2000))
    assert ModelEMA(m, decay=0.5).decay(4000) == 0.5 * (1 - math.exp(-2))


def test_ema_desc_layout_matches_the_c_compiler(tmp_path):
    from dyk import lib
    src = tmp_path / "probe.c"
    cls = lib.DykEmaDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dyk_hip.h"', "int main(void){",
             'printf("sizeof %zu\\n", sizeof(DykEmaDesc));', 'printf("max %d\\n", DYK_EMA_MAX_REGIONS);']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(DykEmaDesc, %s));' % (f, f))
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(cls)
    assert int(out["max"]) == lib.EMA_MAX_REGIONS
    for f, _ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f


def _desc(n=(64, 8), src=(0x10000, 0x20000), dst=(0x30000, 0x40000)):
    from dyk import lib
    d = lib.DykEmaDesc()
    for r in range(len(n)):
        d.src[r], d.dst[r], d.n[r] = src[r], dst[r], n[r]
    d.nregions = len(n)
    d.d, d.omd = 0.5, 0.5
    return d


@pytest.mark.parametrize("bad", ["null", "nregions0", "nregions5", "src_null", "dst_null", "src_misaligned",
                                 "dst_misaligned", "n_zero", "n_negative", "n_not_4"])
def test_bad_descriptors_are_rejected_before_any_launch(bad):
    """the argument checks of dyk_ema_update run before anything touches the device (no GPU here: a launch would fail with
    DYK_ERR_HIP, not DYK_ERR_ARG).  The addresses are never dereferenced."""
    from dyk import lib
    h = lib.load()
    if bad == "null":
        assert h.dyk_ema_update(None, None) == -1
        return
    d = _desc()
    if bad == "nregions0":
        d.nregions = 0
    elif bad == "nregions5":
        d.nregions = lib.EMA_MAX_REGIONS + 1
    elif bad == "src_null":
        d.src[1] = None
    elif bad == "dst_null":
        d.dst[0] = None
    elif bad == "src_misaligned":
        d.src[1] = 0x20004
    elif bad == "dst_misaligned":
        d.dst[0] = 0x30008
    elif bad == "n_zero":
        d.n[1] = 0
    elif bad == "n_negative":
        d.n[0] = -64
    elif bad == "n_not_4":
        d.n[1] = 6
    assert h.dyk_ema_update(ctypes.byref(d), None) == -1


def test_deepcopy_of_a_never_run_model_is_independent():
    m = _yolo()
    assert m._engine is None
    c = copy.deepcopy(m)
    assert c._engine is None and type(c) is type(m)
    sm, sc = m.state_dict(), c.state_dict()
    assert list(sm) == list(sc)
    for k in sm:
        assert torch.equal(sm[k], sc[k]), k
        assert sm[k].untyped_storage().data_ptr() != sc[k].untyped_storage().data_ptr(), k
    with torch.no_grad():
        next(c.parameters()).add_(1.0)
    assert not torch.equal(next(c.parameters()), next(m.parameters()))
    # an engine created (but not run) stays with the original
    m.engine
    c2 = copy.deepcopy(m)
    assert c2._engine is None and m._engine is not None
    assert c2.engine is not m.engine and c2.engine.store.entries[0].param is next(c2.parameters())


def test_deepcopy_leaves_the_loss_runtime_state_behind():
    """compute_loss keeps per-model runtime state in `_dyk_*` attributes (pending device-flag copies and their HIP events,
    dyk/detect.py): not copyable, and not the copy's"""
    import threading
    m = _yolo()
    m.nc, m.hyp = 1, {"iou_t": 0.2}
    m.__dict__["_dyk_loss_flags"] = [(torch.zeros(1), threading.Lock(), None)]      # (an Event does not copy either)
    m.__dict__["_dyk_anchor_cache"] = {0: [1.0, 2.0]}
    c = copy.deepcopy(m)
    assert not [k for k in c.__dict__ if k.startswith("_dyk_")]
    assert c.nc == 1 and c.hyp == m.hyp and c.hyp is not m.hyp
    assert [conv._dyk_stem for conv in c.modules() if isinstance(conv, torch.nn.Conv2d)] == \
        [conv._dyk_stem for conv in m.modules() if isinstance(conv, torch.nn.Conv2d)]


def test_deepcopy_of_an_adopted_model_gets_compact_tensors_of_its_own():
    """after the first forward the parameters and BatchNorm buffers are views into the flat buffers P / R / NBT
    (ParamStore.adopt, here on the host): the copy's tensors own their storage, sized to their own values"""
    m = _yolo()
    st = m.engine.store
    st.adopt(torch.device("cpu"))
    c = copy.deepcopy(m)
    assert c._engine is None
    sm, sc = m.state_dict(), c.state_dict()
    for k in sm:
        assert torch.equal(sm[k], sc[k]), k
        t = sc[k]
        assert t.untyped_storage().nbytes() == t.numel() * t.element_size(), k
    for p in c.parameters():
        assert not (st.P.data_ptr() <= p.data_ptr() < st.P.data_ptr() + 4 * st.total)
    assert [p.requires_grad for p in c.parameters()] == [p.requires_grad for p in m.parameters()]


def test_cpu_device_and_cpu_update_are_refused():
    from build_utils.torch_utils import ModelEMA
    from dyk.lib import DykError
    m = _yolo()
    with pytest.raises(DykError, match="no CPU"):
        ModelEMA(m, device="cpu")
    with pytest.raises(DykError, match="no CPU"):
        ModelEMA(m, device=torch.device("cpu"))
    ema = ModelEMA(m)                      # a model still on the CPU: allowed ...
    with pytest.raises(DykError, match="no CPU fallback"):
        ema.update(m)                      # ... its update is not
    assert ema.updates == 0


def test_update_attr_copies_the_public_attributes():
    from build_utils.torch_utils import ModelEMA
    m = _yolo()
    ema = ModelEMA(m)
    m.nc, m.hyp, m.gr = 1, {"giou": 3.54}, 1.0
    m.engine
    ema.update_attr(m)
    assert ema.ema.nc == 1 and ema.ema.hyp is m.hyp and ema.ema.gr == 1.0
    assert ema.ema._engine is not m._engine


def test_a_model_of_another_layout_is_refused():
    from build_utils.torch_utils import ModelEMA
    from dyk.lib import DykError
    ema = ModelEMA(_yolo("kaist_dyolov3_add_sl"))
    with pytest.raises(DykError, match="different parameter-store layouts"):
        ema.update(_yolo("kaist_yolov3"))


@pytest.mark.parametrize("name", ["kaist_yolov3", "kaist_dyolov3_add_sl", "kaist_dyolov4_fshare_global_concat_se3",
                                  "kaist_dyolov4_mobilenetv3_fshare_global_cse3",
                                  "kaist_dyolov4_mobilenetv2_fshare_global_cse3", "kaist_dyolov3_concat_inc"])
def test_flat_buffers_cover_every_floating_state_dict_entry(name):
    """the one launch of ModelEMA.update covers P and R: every floating entry the reference's loop visits is in one of them"""
    from dyk.ema import FlatEMA
    m = _yolo(name)
    c = copy.deepcopy(m)
    FlatEMA().check_layout(c, m)            # raises on a layout difference or an entry outside the flat buffers
    st = m.engine.store
    n_float = sum(1 for v in m.state_dict().values() if v.dtype.is_floating_point)
    assert n_float == len(st.entries) + len(st.rstats)
