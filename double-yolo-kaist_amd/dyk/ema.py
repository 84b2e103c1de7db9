"""Exponential moving average of a model's weights over the flat parameter store: the native half of
build_utils.torch_utils.ModelEMA (reference build_utils/torch_utils.py:77-126).

The reference walks the shadow's state_dict and runs ~3 torch kernels per floating entry (1114 entries on the target cfg).
Here every parameter of a YOLO model lives in one flat fp32 buffer P and every BatchNorm running statistic in a second one, R
(dyk/params.py), and the shadow is a deepcopy of the model, so its ParamStore has the same layout: one dyk_ema_update launch
updates the shadow's P and R from the model's, element by element (the zero padding between entries stays zero).
Non-floating entries (num_batches_tracked) are not touched, as in the reference.
"""
import ctypes

import torch

from . import lib as L
from .lib import check, load


def launch(pairs, d, stream=None):
    """dst = fl32(fl32(dst * fl32(d)) + fl32(fl32(1 - d) * src)) for every (src, dst) pair of contiguous fp32 CUDA tensors, in ONE
    launch on `stream` (default: the current stream).  `d` is a Python float: it is rounded to fp32, and `1 - d` is formed in
    double first, as torch does for `v *= d; v += (1. - d) * m`."""
    if not 1 <= len(pairs) <= L.EMA_MAX_REGIONS:
        raise L.DykError("dyk_ema_update takes 1 to %d regions, got %d" % (L.EMA_MAX_REGIONS, len(pairs)))
    desc = L.DykEmaDesc()
    for r, (src, dst) in enumerate(pairs):
        for t in (src, dst):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise L.DykError("dyk_ema_update reads and writes contiguous float32 CUDA tensors (got %s %s)" % (t.dtype, t.device))
        if src.numel() != dst.numel() or src.device != dst.device:
            raise L.DykError("dyk_ema_update: region %d pairs %d elements on %s with %d on %s"
                             % (r, src.numel(), src.device, dst.numel(), dst.device))
        desc.src[r], desc.dst[r], desc.n[r] = src.data_ptr(), dst.data_ptr(), src.numel()
    desc.nregions = len(pairs)
    desc.d, desc.omd = float(d), 1.0 - float(d)
    if stream is None:
        stream = torch.cuda.current_stream(pairs[0][1].device)
    check(load().dyk_ema_update(ctypes.byref(desc), ctypes.c_void_p(stream.cuda_stream)), "dyk_ema_update")


def _layout(model, st):
    """what the flat buffers hold, by state_dict key: (parameters, running statistics, total, rtotal)"""
    names = {id(m): n for n, m in model.named_modules()}
    params = tuple((e.name, e.offset, e.numel) for e in st.entries)
    stats = tuple(("%s.%s" % (names[id(m)], attr), roff, n) for m, attr, roff, n in st.rstats)
    return params, stats, st.total, st.rtotal


class FlatEMA:
    """`update(ema_model, model, d)`: the shadow's P and R move towards the model's by decay d (one launch on the current
    stream), then the shadow's compute-dtype weight copies are marked stale: the kernel writes P through a raw pointer, which
    bumps no Parameter version counter (ParamStore.version_key)."""

    def __init__(self):
        self._checked = None            # (model store, shadow store) whose layouts were found identical

    def check_layout(self, ema_model, model):
        """DykError unless the two models' flat buffers hold the same entries at the same offsets, and every floating
        state_dict entry of the model is one of them (no entry the one launch would miss).  Host only; cached per store pair."""
        src, dst = model.engine.store, ema_model.engine.store
        if self._checked is not None and self._checked[0] is src and self._checked[1] is dst:
            return src, dst
        a, b = _layout(model, src), _layout(ema_model, dst)
        if a != b:
            diff = [(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]) if x != y][:1]
            raise L.DykError("ModelEMA: the model and its EMA have different parameter-store layouts (%d / %d parameters, "
                             "%d / %d running statistics, total %d / %d, rtotal %d / %d%s): the EMA must be a copy of this model"
                             % (len(a[0]), len(b[0]), len(a[1]), len(b[1]), a[2], b[2], a[3], b[3],
                                ", first difference %s / %s" % diff[0] if diff else ""))
        covered = {k for k, _, _ in a[0] + a[1]}
        missed = [k for k, v in model.state_dict().items() if v.dtype.is_floating_point and k not in covered]
        if missed:
            raise L.DykError("ModelEMA: floating state_dict entries outside the flat buffers: %s" % missed[:4])
        self._checked = (src, dst)
        return src, dst

    def update(self, ema_model, model, d):
        src, dst = self.check_layout(ema_model, model)
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise L.DykError("ModelEMA.update runs on the MI355X HIP path only: move the model to a cuda device (got %s). "
                             "There is no CPU fallback." % dev)
        edev = next(ema_model.parameters()).device
        if edev != dev:
            raise L.DykError("ModelEMA.update: the EMA is on %s, the model on %s: keep both on the same GPU" % (edev, dev))
        for m, st in ((model, src), (ema_model, dst)):
            if not st.is_adopted(dev):          # as the first forward pass does (Engine._prepare)
                st.adopt(dev)
                m.engine.plans = {}
        launch([(src.P, dst.P), (src.R, dst.R)], d)
        dst.mark_dirty()
