"""Fused optimizers over the flat parameter store (one HIP launch per step for the whole model).

Drop-in for the torch.optim.Adam / SGD(nesterov) instances reference train.py:85-91 builds: same update
rule, same constructor arguments, `step()` / `zero_grad()` / `param_groups[0]['lr']` for LR schedulers,
`state_dict()` / `load_state_dict()` in torch.optim's own per-parameter format (the reference checkpoint stores
`optimizer.state_dict()`, train.py:229), and -- like `pg = [p for p in model.parameters() if p.requires_grad]`
(train.py:84) -- no update of parameters frozen with `requires_grad_(False)` (`--freeze-layers`, train.py:77-82).

Opt-in protection (`max_grad_norm=`, `skip_nonfinite=`): what the reference harness gets from amp.GradScaler
(train_utils/kaist_train_eval_utils.py:44,103-108) and torch.nn.utils.clip_grad_norm_, decided on the device from one
reduction over the flat gradient buffer (csrc/optim_guard.hip) -- no per-tensor kernels, no host synchronisation.  The step
reads the decision from a small device record; FusedAdam and FusedSGD share one step() that picks the library entry from
(update rule, parameter groups or not, record or not).

Parameter groups (`param_groups=`, torch.optim's list of dicts) and decoupled weight decay (`decoupled_weight_decay=`,
`FusedAdamW`): up to 8 groups with their own `lr` / `weight_decay`, still one launch -- the byte per element that marks frozen
parameters carries the group index (dyk_adam_step_groups / dyk_sgd_step_groups, csrc/optim.hip), and the groups' hyper-parameters
travel as a kernel argument that is rebuilt from `param_groups` at every step, so LR schedulers and warm-up code that write
`group['lr']` work as with torch.optim.  `yolo_param_groups(model, weight_decay)` builds the usual detector recipe: decay on
weights of dimension >= 2 only.  One L2 group -- every caller that passes no groups -- takes the entries it always took.
"""
import ctypes
import os
import struct

import numpy as np
import torch

from . import lib as L
from .lib import check, load

MAX_GROUPS = L.OPT_MAX_GROUPS
_SHARED_KEYS = ("betas", "eps", "momentum", "nesterov", "dampening")     # one value for all groups (DykOptimDesc carries them)


def _fl32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _entry_fields(e):
    return (e.offset, e.numel, e.param) if hasattr(e, "offset") else e


def group_map(entries, groups, total):
    """The byte per element of the flat buffer that the grouped step kernels read: k on the elements of every parameter of
    groups[k-1] that requires a gradient, 0 elsewhere (frozen parameters, parameters of no group, the padding behind every
    entry).  entries: (offset, numel, param) records, or the ParamStore's entries; groups: dicts with 'params', as
    optimizer.param_groups.  Entries start at multiples of 64 elements, so the four bytes of a 16-byte vector agree.
    -> numpy uint8 array of `total` bytes"""
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError("1 to %d parameter groups, got %d" % (MAX_GROUPS, len(groups)))
    index = {}
    for k, g in enumerate(groups, 1):
        for p in g["params"]:
            if id(p) in index:
                raise ValueError("a parameter appears in more than one parameter group (groups %d and %d)" % (index[id(p)] - 1, k - 1))
            index[id(p)] = k
    out = np.zeros(total, np.uint8)
    for e in entries:
        off, n, p = _entry_fields(e)
        if off % 4 or off < 0 or off + n > total:
            raise ValueError("entry [%d, %d) does not fit a buffer of %d elements in whole 16-byte vectors" % (off, off + n, total))
        if p.requires_grad:
            out[off:off + n] = index.get(id(p), 0)
    return out


def trainable_mask(st):
    """None when every parameter of the store is trainable, else a byte per element of the flat buffer on its device (1 = update):
    frozen parameters get neither the update nor weight decay nor moments -- group_map with the trainable parameters as one group"""
    if not st.frozen_key():
        return None
    live = [dict(params=[e.param for e in st.entries if e.param.requires_grad])]
    return torch.from_numpy(group_map(st.entries, live, st.total)).to(st.P.device)


def _rec_field(rec, name, dtype):
    """one field of a DykGradGuardRec held as device bytes, as a one-element tensor view"""
    f = getattr(L.DykGradGuardRec, name)
    return rec[f.offset:f.offset + f.size].view(dtype)


def yolo_param_groups(model, weight_decay, bias_lr=None):
    """The three parameter groups of the YOLOv3/v4 training recipe over the trainable parameters of `model`:
      0  weights of dimension >= 2 (convolution, depthwise, SE fully-connected): weight_decay
      1  BatchNorm scale / shift and WeightedFeatureFusion.w: no decay
      2  biases of every other module: no decay, `lr` = bias_lr when given (the warm-up schedule of the biases)
    Frozen parameters (requires_grad False) are left out.  For FusedAdam / FusedSGD(param_groups=...) or torch.optim."""
    import torch.nn as nn
    decay, plain, biases = [], [], []
    seen = set()
    for mod in model.modules():
        for name, p in mod.named_parameters(recurse=False):
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            if isinstance(mod, nn.modules.batchnorm._NormBase):
                plain.append(p)
            elif name == "bias":
                biases.append(p)
            elif p.dim() >= 2:
                decay.append(p)
            else:
                plain.append(p)
    groups = [dict(params=decay, weight_decay=float(weight_decay)), dict(params=plain, weight_decay=0.0),
              dict(params=biases, weight_decay=0.0)]
    if bias_lr is not None:
        groups[2]["lr"] = float(bias_lr)
    return groups


def _checked_groups(model, param_groups, defaults):
    """param_groups as torch.optim takes them, checked: at most 8, a partition of the trainable parameters of `model`, no
    per-group value of a hyper-parameter the kernels share"""
    groups = []
    for g in param_groups:
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError("param_groups must be a list of dicts with a 'params' entry")
        ps = g["params"]
        g = dict(g, params=[ps] if isinstance(ps, torch.Tensor) else list(ps))
        for k in _SHARED_KEYS:
            if k in g and k in defaults:
                same = tuple(g[k]) == tuple(defaults[k]) if k == "betas" else g[k] == defaults[k]
                if not same:
                    raise ValueError("parameter groups share %r (%r); a group asks for %r" % (k, defaults[k], g[k]))
        unknown = [k for k in g if k not in defaults and k != "params"]
        if unknown:
            raise ValueError("unknown parameter-group option(s) %s" % unknown)
        groups.append(g)
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError("1 to %d parameter groups, got %d" % (MAX_GROUPS, len(groups)))
    names = {id(p): n for n, p in model.named_parameters()}
    trainable = [p for p in model.parameters() if p.requires_grad]
    want = {id(p) for p in trainable}
    seen = set()
    for k, g in enumerate(groups):
        for p in g["params"]:
            if id(p) in seen:
                raise ValueError("parameter %s appears in more than one parameter group" % names.get(id(p), "<not of this model>"))
            if id(p) not in want:
                raise ValueError("group %d holds %s, which is not a trainable parameter of the model" % (
                    k, names.get(id(p), "a tensor")))
            seen.add(id(p))
    for p in trainable:
        if id(p) not in seen:
            raise ValueError("trainable parameter %s is in no parameter group" % names[id(p)])
    return groups


class _FusedBase(torch.optim.Optimizer):
    _state_names = ()            # torch.optim state entries that map onto the flat buffers (m, v)
    _rule = None                 # "adam" / "sgd": the library entries are dyk_<rule>_step, ..._guarded, ..._groups

    def _hyper(self, d):
        """writes the rule's shared hyper-parameters into the DykOptimDesc `d` -> (beta1, beta2) of the record's bias corrections"""
        raise NotImplementedError

    def __init__(self, model, defaults, max_grad_norm=None, skip_nonfinite=False, param_groups=None):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (0.0 < max_grad_norm < float("inf")):
                raise ValueError("max_grad_norm must be a positive finite number or None, got %r" % (max_grad_norm,))
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guarded = self.skip_nonfinite or max_grad_norm is not None
        self._rec = self._stats_ws = None            # device record / workspace of the guarded mode (never allocated otherwise)
        self._stats_ring, self._stats_pending, self._stats_last = None, [], None
        self.model = model
        params = [p for p in model.parameters() if p.requires_grad]
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        super().__init__(params if param_groups is None else _checked_groups(model, param_groups, defaults), defaults)
        self._t = 0
        self._m = self._v = None
        self._mask, self._mask_key = None, None
        self._gmap, self._gmap_key = None, None      # grouped mode: the byte per element that names the group
        self._step_mask = None                       # the mask the last _desc() handed to the kernel
        self.grad_scale = 1.0
        self.zero_in_step = True
        self._side = None
        self._buckets = None
        self._fresh = True
        mode = os.environ.get("DYK_OPT_OVERLAP", "1")
        self.early_start = mode == "early"
        if mode != "0":
            from .ddp import GradAllReduce
            model.engine.opt_overlap = GradAllReduce(model, None, attach=False)
            model.engine.opt_early = self.early_start

    def _store(self):
        st = self.model.engine.store
        if st.P is None:
            raise L.DykError("run one forward pass (or model.engine.store.adopt(device)) before optimizer.step()")
        return st

    def zero_grad(self, set_to_none=False):
        """Clears the flat gradient buffer unless it is known to be clean: a fused step that ran AFTER the last
        backward has already zeroed it.  A step skipped by GradScaler (inf/NaN gradients) or by the caller leaves
        `store.grads_dirty` set, so the stale gradients are dropped here as with torch.optim."""
        st = self.model.engine.store
        if st.G is not None:
            st.attach_grads()
            if st.grads_dirty:
                st.G.zero_()
                st.grads_dirty = False

    def _buffers(self, st):
        if self._m is None or self._m.device != st.P.device:
            self._m = torch.zeros_like(st.P)
            self._v = torch.zeros_like(st.P) if "exp_avg_sq" in self._state_names else None
            self._fresh = True            # (their fill runs on the caller's stream: the side stream of _launch must see it)
        return self._m, self._v

    def _trainable_mask(self, st):
        """None when every parameter is trainable, else a byte per element of the flat buffer (1 = update):
        frozen parameters get neither the update nor weight decay nor moments."""
        key = st.frozen_key()
        if key != self._mask_key:
            self._mask_key = key
            self._mask = trainable_mask(st)
            if self._mask is not None:
                self._fresh = True
        return self._mask

    def _grouped(self):
        """more than one group, or decoupled decay: the `_groups` entries of the library.  One L2 group takes the entries, the
        launches and the mask it always took."""
        return len(self.param_groups) > 1 or any(g.get("decoupled_weight_decay", False) for g in self.param_groups)

    def _group_map(self, st):
        key = (st.frozen_key(), tuple(tuple(id(p) for p in g["params"]) for g in self.param_groups))
        if key != self._gmap_key or self._gmap.device != st.P.device:
            self._gmap_key = key
            self._gmap = torch.from_numpy(group_map(st.entries, self.param_groups, st.total)).to(st.P.device)
            self._fresh = True
        return self._gmap

    def _group_table(self):
        """DykOptimGroups from param_groups as they are NOW (a scheduler may have written lr since the last step)"""
        t = L.DykOptimGroups()
        t.count = len(self.param_groups)
        for k, g in enumerate(self.param_groups):
            r = t.g[k]
            r.lr, r.weight_decay = float(g["lr"]), float(g["weight_decay"])
            r.decay_mul = _fl32(1.0 - _fl32(_fl32(r.lr) * _fl32(r.weight_decay)))
            r.flags = L.OPT_GROUP_DECOUPLED if g.get("decoupled_weight_decay", False) else 0
        return t

    def _take_buckets(self, works, total):
        """GradAllReduce.all_reduce(optimizer=self): [(work, lo, hi)] of the data-parallel exchange; accepted when the ranges tile
        the flat buffer in whole 8-element groups (else the caller waits as usual)"""
        spans = sorted((lo, hi) for _, lo, hi in works)
        ok = spans and spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        if not ok or any(lo % 8 for lo, _ in spans):
            return False
        self._buckets = list(works)
        return True

    def _launch(self, fn, name, d, buckets, wait_for_main):
        """one launch over the whole flat buffer -- or, when the last backward left an event behind its first segment
        (engine._early: gradients of G[lo:] final, single GPU), two: [lo, total) on a side stream as soon as that event has
        passed (wait_for_main: as soon as everything the caller has enqueued has), [0, lo) behind the backward on the caller's
        stream, which then waits for the side stream.  Same arithmetic per element; the 0.66 ms HBM-bound step of the target cfg
        no longer runs alone after the backward's tail.  buckets: those of _take_buckets, or None."""
        eng = self.model.engine
        early, eng._early = eng._early, None
        main = torch.cuda.current_stream()
        if buckets is None and (early is None or self.model.engine.grad_sync is not None):
            check(fn(ctypes.byref(d), ctypes.c_void_p(main.cuda_stream)), name)
            return
        n = d.n
        if self._side is None:
            # library stream 3 of the schedule runtime (dyk_sched_stream), not a fifth stream: the HIP runtime maps all streams
            # of the process onto four hardware queues and a fifth one shares a queue with whichever stream the runtime picks
            # (in-call, round 4: 28.39 / 28.47 ms with a stream of its own, 28.19 / 28.31 on library stream 3, 28.39 / 28.32 on 2,
            # 28.60 / 28.47 on 1 -- stream 1 carries the second backbone)
            h = ctypes.c_void_p()
            check(load().dyk_sched_stream(3, ctypes.byref(h)), "dyk_sched_stream")
            self._side = torch.cuda.ExternalStream(h.value)
        side = self._side

        def sub(off, cnt):
            e = L.DykOptimDesc()
            ctypes.memmove(ctypes.byref(e), ctypes.byref(d), ctypes.sizeof(L.DykOptimDesc))
            e.p, e.g, e.m = d.p + 4 * off, d.g + 4 * off, d.m + 4 * off
            e.v = d.v + 4 * off if d.v else None
            e.mask = d.mask + off if d.mask else None
            e.wc = d.wc + 2 * off if d.wc else None
            e.n = cnt
            return e
        if self._fresh:
            # moment buffers / trainable mask were created (filled on the caller's stream) for this very step: the side stream
            # waits for the caller's stream once -- the first step runs without the overlap
            first = torch.cuda.Event()
            first.record(main)
            side.wait_event(first)
            self._fresh = False
        if buckets is not None:
            # data parallel: every bucket's range on the side stream behind ITS all-reduce (Work.wait() orders the current stream
            # behind the collective, it does not block the host); the caller's stream joins at the end
            for w, lo, hi in buckets:
                with torch.cuda.stream(side):
                    w.wait()
                check(fn(ctypes.byref(sub(lo, hi - lo)), ctypes.c_void_p(side.cuda_stream)), name)
            done = torch.cuda.Event()
            done.record(side)
            main.wait_event(done)
            return
        ev, lo = early
        if not wait_for_main and ev is not None:
            # opt-in (DYK_OPT_OVERLAP=early / optimizer.early_start = True): the side stream waits for the event recorded in the
            # MIDDLE of the backward pass only.  Anything the caller enqueued on its own stream between backward() and step() that
            # touches gradients -- clip_grad_norm_, manual scaling, gradient-norm logging -- is NOT ordered against it (a clip
            # would be ignored for G[lo:], a norm could read zeros).  For loops that call step() straight after backward().
            side.wait_event(ev)
        else:
            # default: behind EVERYTHING the caller has enqueued so far: the two ranges still run side by side
            # and the transposed packs are rebuilt beside the next forward
            now = torch.cuda.Event()
            now.record(main)
            side.wait_event(now)
        check(fn(ctypes.byref(sub(lo, n - lo)), ctypes.c_void_p(side.cuda_stream)), name)
        done = torch.cuda.Event()
        done.record(side)
        check(fn(ctypes.byref(sub(0, lo)), ctypes.c_void_p(main.cuda_stream)), name)
        main.wait_event(done)

    def _desc(self, st):
        m, v = self._buffers(st)
        g = self.param_groups[0]
        d = L.DykOptimDesc()
        d.p, d.g, d.m = st.P.data_ptr(), st.G.data_ptr(), m.data_ptr()
        d.v = v.data_ptr() if v is not None else None
        d.n = st.total
        d.lr, d.weight_decay, d.grad_scale = float(g["lr"]), float(g["weight_decay"]), float(self.grad_scale)
        d.zero_grad = 1 if self.zero_in_step else 0
        if self._grouped():
            mask = self._group_map(st)               # (always there: the frozen-overwritten rule below applies)
            d.lr = d.weight_decay = 0.0              # (ignored by the _groups entries: DykOptimGroups carries them)
        else:
            mask = self._trainable_mask(st)
        self._step_mask = mask
        d.mask = mask.data_ptr() if mask is not None else None
        bf = st._compute.get(torch.bfloat16)
        d.wc = bf["Wc"].data_ptr() if bf is not None else None
        # the kernel writes the bf16 copy of the elements it updates and skips frozen ones: their copy is still right afterwards
        # only if it was current when the step began (a frozen tensor overwritten since the last forward -- load_state_dict,
        # load_darknet_weights -- needs the full cast).  Without a mask every element is written.
        self._wc_complete = bf is not None and (mask is None or bf["version"] == st.version_key())
        return d, bf

    # ------------------------------------------------------------------ guarded mode (max_grad_norm / skip_nonfinite)
    def _guard_record(self, st):
        if self._rec is None or self._rec.device != st.P.device:
            from . import ops
            if self._rec is not None:        # the model moved: carry the applied count over
                self.grad_stats(wait=True)
            self._rec = ops.grad_guard_record(st.P.device)
            self._stats_ws = ops.grad_stats_workspace(st.total, st.P.device)
            self._stats_ring = [torch.zeros(8, ops.GRAD_REC_BYTES, dtype=torch.uint8).pin_memory(), 0]
            if self._t:                      # a checkpoint was loaded before the first step
                _rec_field(self._rec, "applied", torch.int32)[0] = self._t
            self._fresh = True
        return self._rec

    def _decide(self, st, d, bf, betas, buckets):
        """guarded mode, before the step: dyk_grad_stats over the whole G on the caller's stream (behind everything enqueued so
        far: the backward, a data-parallel all-reduce) and the record's asynchronous copy to pinned memory -> the record, which
        the step -- one launch or the two ranges of _launch -- reads.  With data-parallel buckets the norm needs all of G: the
        caller's stream waits for every bucket first and the bucket-wise overlap is given up (every rank holds the same G
        afterwards and reaches the same decision without a further collective)."""
        from . import ops
        for w, _, _ in buckets or ():
            w.wait()
        rec = self._guard_record(st)
        if self.skip_nonfinite:
            # a skipped step writes no bf16 copy at all: the cast may be left out only if the copy was current before the step
            self._wc_complete = bf is not None and bf["version"] == st.version_key()
        # (_desc has refreshed _step_mask; in grouped mode it is the group map: live = byte != 0)
        ops.grad_stats(st.G, rec, self._stats_ws, mask=self._step_mask, grad_scale=d.grad_scale, max_norm=self.max_grad_norm or 0.0,
                       beta1=betas[0], beta2=betas[1], skip_nonfinite=self.skip_nonfinite)
        self._publish_stats(rec)
        return rec

    def _entry(self, rec):
        """the library entry of (rule, grouped, with a record) with the group table and the record bound
        -> (callable(descriptor reference, stream), its name for `check`)"""
        grouped = self._grouped()
        name = "dyk_%s_step%s" % (self._rule, "_groups" if grouped else "_guarded" if rec is not None else "")
        fn = getattr(load(), name)
        rp = ctypes.c_void_p(rec.data_ptr()) if rec is not None else None
        if grouped:
            table = self._group_table()
            return (lambda dref, stream: fn(dref, ctypes.byref(table), rp, stream)), name
        if rec is not None:
            return (lambda dref, stream: fn(dref, rp, stream)), name
        return fn, name

    @torch.no_grad()
    def step(self, closure=None):
        st = self._store()
        self._check_loss_flag()
        st.attach_grads()
        if not self._guarded:                # (guarded: the record counts the steps that were applied)
            self._t += 1
        d, bf = self._desc(st)
        betas = self._hyper(d)
        d.step = 0 if self._guarded else self._t
        buckets, self._buckets = self._buckets, None
        rec = None
        if self._guarded:
            rec, buckets = self._decide(st, d, bf, betas, buckets), None
        fn, name = self._entry(rec)
        # (with a record the side stream must wait for the statistics, which run on the caller's stream)
        self._launch(fn, name, d, buckets, wait_for_main=rec is not None or not self.early_start)
        self._finish(st, bf)

    def _publish_stats(self, rec):
        ring, pend = self._stats_ring, self._stats_pending
        self._poll_stats()
        if len(pend) >= ring[0].shape[0]:        # the host runs a whole ring ahead of the device: wait for the oldest copy
            pend[0][1].synchronize()
            self._poll_stats()
        host = ring[0][ring[1] % ring[0].shape[0]]
        ring[1] += 1
        host.copy_(rec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        pend.append((host, ev))

    def _poll_stats(self):
        from . import ops
        pend = self._stats_pending
        while pend and pend[0][1].query():
            host, _ = pend.pop(0)
            r = ops.grad_record_from_bytes(host.numpy().tobytes())
            self._stats_last = dict(norm=float(r.norm), clip_coef=float(r.coef), nonfinite=int(r.nonfinite),
                                    applied_steps=int(r.applied), skipped_steps=int(r.skipped))
            self._t = int(r.applied)

    def grad_stats(self, wait=False):
        """{norm, clip_coef, nonfinite, applied_steps, skipped_steps} of the newest guarded step whose record has reached the
        host (norm is that of grad * grad_scale over the trainable parameters), or None.  wait=False never synchronises: the
        answer may be a step or two old.  wait=True waits for the copy behind the last step()."""
        if wait and self._stats_pending:
            self._stats_pending[-1][1].synchronize()
        if self._stats_pending:
            self._poll_stats()
        return None if self._stats_last is None else dict(self._stats_last)

    def _check_loss_flag(self):
        """the reference raises IndexError inside compute_loss when a target lies on the right / bottom image edge
        (grid index == grid size: build_utils/utils.py:370 with :248); the HIP loss records that in a device flag
        which dyk.detect copies to pinned host memory asynchronously.  Flags whose copy has completed are examined
        here (no host synchronisation: the error surfaces one optimizer step late at most)."""
        from .detect import raise_if_target_outside_grid
        raise_if_target_outside_grid(self.model, wait=False)

    def _finish(self, st, bf):
        if self.zero_in_step:
            st.grads_dirty = False
        st.mark_dirty()
        if bf is not None:                # the bf16 copy was written by the step kernel: refresh the rest only
            side = self._side
            st.compute_weights(torch.bfloat16, skip_cast=self._wc_complete, side=side)
        for dt in list(st._compute):
            # (the fp16 copy serves inference plans only: mark_dirty() above made it stale, and the next fp16 forward rebuilds it
            # through the version check of compute_weights -- no cast per training step for a copy an evaluation left behind)
            if dt not in (torch.bfloat16, torch.float16):
                st.compute_weights(dt)

    # ------------------------------------------------------------------ checkpoint format of torch.optim
    def _export_state(self):
        st = self.model.engine.store
        if self._m is None or st.P is None:
            return
        by_param = {id(e.param): e for e in st.entries}
        flats = dict(zip(self._state_names, (self._m, self._v)))
        for g in self.param_groups:
            for p in g["params"]:
                e = by_param[id(p)]
                s = {"step": torch.tensor(float(self._t))}
                for name, flat in flats.items():
                    s[name] = st._view(flat, e)
                self.state[p] = s

    def state_dict(self):
        if self._guarded and self._rec is not None:
            self.grad_stats(wait=True)       # step = steps actually applied (a skipped step does not advance Adam's t)
        self._export_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        decoupled = [g.get("decoupled_weight_decay") for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, flag in zip(self.param_groups, decoupled):
            if flag is not None:
                g.setdefault("decoupled_weight_decay", flag)      # (a checkpoint of a torch without that option)
        st = self._store()
        m, v = self._buffers(st)
        flats = dict(zip(self._state_names, (m, v)))
        by_param = {id(e.param): e for e in st.entries}
        steps = set()
        loaded = False
        with torch.no_grad():
            for p, s in list(self.state.items()):
                e = by_param[id(p)]
                for name, flat in flats.items():
                    if name in s and s[name] is not None:
                        st._view(flat, e).copy_(s[name].to(flat.device, torch.float32))
                        loaded = True
                if "step" in s:
                    steps.add(int(float(s["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): the fused step keeps one counter" % sorted(steps))
        # torch.optim.SGD keeps only 'momentum_buffer' (no 'step'): a checkpoint that carries buffers is past its first
        # step -- with _t = 0 the next step would take the first-step branch (m = g) and drop the loaded momentum
        self._t = steps.pop() if steps else (1 if loaded else 0)
        if self._rec is not None:
            self.grad_stats(wait=True)       # (copies of earlier steps must not overwrite _t afterwards)
            _rec_field(self._rec, "applied", torch.int32)[0] = self._t
        self.state.clear()               # the flat buffers are the state; views are rebuilt on demand
        self._fresh = True               # (the copies above ran on the caller's stream)


class FusedAdam(_FusedBase):
    _state_names = ("exp_avg", "exp_avg_sq")
    _rule = "adam"

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False, param_groups=None, decoupled_weight_decay=False):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                     decoupled_weight_decay=bool(decoupled_weight_decay)), max_grad_norm, skip_nonfinite, param_groups)

    def _hyper(self, d):
        g = self.param_groups[0]
        d.beta1, d.beta2, d.eps = float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        return d.beta1, d.beta2


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: FusedAdam with decoupled weight decay (p *= 1 - lr * weight_decay before the Adam update)"""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(model, lr, betas, eps, weight_decay, decoupled_weight_decay=True, **kw)


class FusedSGD(_FusedBase):
    _state_names = ("momentum_buffer",)
    _rule = "sgd"

    def __init__(self, model, lr=1e-3, momentum=0.9, weight_decay=0.0, nesterov=True, max_grad_norm=None,
                 skip_nonfinite=False, param_groups=None):
        if not nesterov:
            raise NotImplementedError("the reference only uses nesterov=True (train.py:88-89)")
        super().__init__(model, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True, dampening=0),
                         max_grad_norm, skip_nonfinite, param_groups)

    def _hyper(self, d):
        d.beta1 = float(self.param_groups[0]["momentum"])
        return 0.0, 0.0


def clip_grad_norm_(model, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ for users of stock torch.optim on the gradient views of a dyk model: one reduction over
    the flat gradient buffer (dyk_grad_stats) and one scaling launch (dyk_grad_scale_by_rec, which stores nothing when the
    norm is within `max_norm`) instead of per-tensor kernels over some 600 views.  Same coefficient as torch,
    max_norm / (norm + 1e-6) clamped to 1, over the trainable parameters; a non-finite norm scales the gradients by it, as
    with error_if_nonfinite=False.  Returns the norm before clipping as a 0-dim tensor on the device (no synchronisation)."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("dyk.optim.clip_grad_norm_ computes the 2-norm only (norm_type=%r)" % (norm_type,))
    max_norm = float(max_norm)
    if not max_norm > 0.0:               # (the kernel reads max_norm <= 0 as "no clipping")
        raise ValueError("max_norm must be positive, got %r" % (max_norm,))
    from . import ops
    m = model.module if hasattr(model, "module") and not hasattr(model, "engine") else model
    st = m.engine.store
    if st.P is None:
        raise L.DykError("run one forward and backward pass before clip_grad_norm_()")
    st.attach_grads()
    state = m.__dict__.get("_dyk_clip")
    key = (st.frozen_key(), st.P.device)
    if state is None or state["key"] != key:
        state = m.__dict__["_dyk_clip"] = dict(key=key, mask=trainable_mask(st), rec=ops.grad_guard_record(st.P.device),
                                               ws=ops.grad_stats_workspace(st.total, st.P.device))
    rec, mask = state["rec"], state["mask"]
    ops.grad_stats(st.G, rec, state["ws"], mask=mask, max_norm=max_norm)
    ops.grad_scale_by_rec(st.G, rec, mask=mask)
    return _rec_field(rec, "norm", torch.float32)[0].clone()
