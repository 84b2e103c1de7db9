"""Small torch helpers the reference keeps in build_utils/torch_utils.py (what the hot path and the unchanged CLI scripts
import: init_seeds, select_device, time_synchronized, model_info; and ModelEMA for training loops that keep EMA weights)."""
import math
import time
from copy import deepcopy

import torch
import torch.nn as nn


def init_seeds(seed=0):
    torch.manual_seed(seed)


def select_device(device="cuda:0"):
    """device string -> torch.device, single GPU or CPU (reference torch_utils.py:35-50)"""
    cpu_request = device.lower() == "cpu"
    if device and not cpu_request:
        assert torch.cuda.is_available(), "CUDA unavailable, invalid device %s requested" % device
    device = torch.device(device)
    if not cpu_request and torch.cuda.is_available():
        di = 0 if device.index is None else device.index
        dp = torch.cuda.get_device_properties(di)
        print("Using torch %s CUDA:%d (%s, %dMB)" % (torch.__version__, di, dp.name, dp.total_memory / 1024 ** 2))
    else:
        print("Using torch %s CPU" % torch.__version__)
    return device


def time_synchronized():
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return time.time()


def model_info(model, verbose=False):
    """parameter / gradient count summary (reference torch_utils.py:53-75)"""
    n_p = sum(x.numel() for x in model.parameters())
    n_g = sum(x.numel() for x in model.parameters() if x.requires_grad)
    if verbose:
        print("%5s %40s %9s %12s %20s" % ("layer", "name", "gradient", "parameters", "shape"))
        for i, (name, p) in enumerate(model.named_parameters()):
            print("%5g %40s %9s %12g %20s" % (i, name.replace("module_list.", ""), p.requires_grad, p.numel(), list(p.shape)))
    print("Model Summary: %g layers, %g parameters, %g gradients" % (len(list(model.parameters())), n_p, n_g))


class ModelEMA:
    """Model Exponential Moving Average (reference torch_utils.py:77-126, after rwightman/pytorch-image-models): `ema` is a
    deepcopy of the model in eval mode whose floating state_dict entries -- parameters and BatchNorm running statistics --
    follow the model's by `v = d * v + (1 - d) * model_v` with the ramp `d = decay * (1 - exp(-updates / 2000))`.  Call
    `update(model)` after every optimizer step, `update_attr(model)` before evaluating `ema`.

    `update` is one HIP launch over the flat parameter and running-statistics buffers (dyk/ema.py), bit-identical to the
    reference's per-entry torch loop.  The shadow lives on the model's GPU: there is no CPU path to evaluate it on, so
    device='cpu' (the reference's way to keep the EMA off the GPU) is refused."""

    def __init__(self, model, decay=0.9999, device=""):
        from dyk.ema import FlatEMA
        from dyk.lib import DykError
        if device and torch.device(device).type == "cpu":
            raise DykError("ModelEMA(device=%r): the EMA model is evaluated on the MI355X HIP path only, which has no CPU "
                           "fallback -- keep it on the model's GPU (device='')" % (device,))
        self.ema = deepcopy(model)
        self.ema.eval()
        self.updates = 0
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))
        self.device = device
        if device:
            self.ema.to(device=device)
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._flat = FlatEMA()

    def update(self, model):
        d = self.decay(self.updates + 1)
        with torch.no_grad():
            parallel = (nn.parallel.DataParallel, nn.parallel.DistributedDataParallel)
            src = model.module if type(model) in parallel else model
            dst = self.ema.module if type(self.ema) in parallel else self.ema
            self._flat.update(dst, src, d)
        self.updates += 1

    def update_attr(self, model):
        # assign attributes (which may change during training)
        for k in model.__dict__.keys():
            if not k.startswith("_"):
                setattr(self.ema, k, getattr(model, k))
