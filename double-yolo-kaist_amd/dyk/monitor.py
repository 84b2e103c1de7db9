"""Per-tensor statistics of the flat parameter store: which tensor's gradient exploded, went non-finite or died.

The fused optimizers' guard (`FusedAdam(skip_nonfinite=True, max_grad_norm=...)`, `optimizer.grad_stats()`) reports ONE norm
and ONE non-finite count for the whole gradient buffer.  `TensorStats` reports them per tensor -- norm, largest magnitude,
non-finite and zero counts for every parameter, its gradient, the optimizer's moments and the BatchNorm running statistics --
from one segmented reduction over the flat buffers (dyk_tensor_stats, csrc/tensor_stats.hip: two launches per table, all
requested buffers in the same pass) instead of a host loop of `p.grad.norm()` / `torch.isfinite(p.grad).all()` over some 600
views with a synchronisation each.  Nothing here runs unless a TensorStats is constructed and launched.

    stats = TensorStats(model, what=("grad", "param"))
    loss.backward()
    stats.launch()                      # between backward() and optimizer.step(): the fused step may clear G
    optimizer.step()
    ...
    r = stats.read()                    # newest result that has reached the host, or None; never synchronises
    if optimizer.grad_stats()["skipped_steps"]:
        print(stats.first_nonfinite(), stats.summary())
"""
import collections
import math

import torch

from . import lib as L
from . import ops

Stat = collections.namedtuple("Stat", "norm absmax nonfinite zeros numel sumsq")

WHAT = ("param", "grad", "exp_avg", "exp_avg_sq", "momentum", "running")
_MOMENTS = {"exp_avg": ("exp_avg", "_m"), "exp_avg_sq": ("exp_avg_sq", "_v"), "momentum": ("momentum_buffer", "_m")}
RING = 8


class TensorStats:
    """what: a subset of "param", "grad", "exp_avg", "exp_avg_sq" (FusedAdam) / "momentum" (FusedSGD), "running".
    The moment names need `optimizer=`, a FusedAdam / FusedSGD of this model, whose flat moment buffers share the store's
    layout; a name that optimizer does not keep raises ValueError.  "running" reads the BatchNorm running statistics with a
    table of their own (a second dyk_tensor_stats call)."""

    def __init__(self, model, what=("grad",), optimizer=None):
        model = model.module if hasattr(model, "module") and not hasattr(model, "engine") else model
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what:
            raise ValueError("TensorStats: nothing to report (what is empty)")
        for w in what:
            if w not in WHAT:
                raise ValueError("TensorStats: unknown quantity %r (one of %s)" % (w, ", ".join(WHAT)))
        if len(set(what)) != len(what):
            raise ValueError("TensorStats: %r names a quantity twice" % (what,))
        for w in what:
            if w in _MOMENTS:
                if optimizer is None:
                    raise ValueError("TensorStats: %r needs optimizer=, a FusedAdam / FusedSGD of this model" % w)
                names = getattr(optimizer, "_state_names", None)
                if names is None or getattr(optimizer, "model", None) is not model:
                    raise ValueError("TensorStats: optimizer= must be a dyk.optim.FusedAdam / FusedSGD of this model")
                if _MOMENTS[w][0] not in names:
                    raise ValueError("TensorStats: %s keeps no %r (it keeps %s)" % (type(optimizer).__name__, w, ", ".join(names)))
        self.model, self.optimizer = model, optimizer
        self.what = what
        self._flat = tuple(w for w in what if w != "running")          # buffers of the parameter table, in `what` order
        self._key = None
        self._tab = self._rtab = None
        self._ring, self._slot = None, 0
        self._pending = []           # (host slot, event, meta), oldest first
        self._last = None            # (bytes, meta) of the newest copy that has landed
        self._decoded = None

    # ------------------------------------------------------------------ tables
    def _tables(self, st):
        key = (st.frozen_key(), st.P.device, st.P.data_ptr())
        if key == self._key:
            return
        dev = st.P.device
        params, running = st.segment_table()
        # frozen parameters have neither gradient nor moments: skipped (flag bit per buffer) for everything but "param"
        skip = sum(1 << k for k, w in enumerate(self._flat) if w != "param")
        frozen = set(key[0])
        self._names = [n for n, _, _ in params]
        self._numels = [n for _, _, n in params]
        self._flags = [skip if n in frozen else 0 for n in self._names]
        self._tab = self._rtab = None
        nrec = 0
        if self._flat:
            self._tab = ops.tensor_stats_worklist([(o, n, f) for (_, o, n), f in zip(params, self._flags)], dev)
            self._ws = ops.tensor_stats_workspace(self._tab["nitems"], len(self._flat), dev)
            nrec += self._tab["nseg"] * len(self._flat)
        self._rnames, self._rnumels = [n for n, _, _ in running], [n for _, _, n in running]
        if "running" in self.what and running:
            self._rtab = ops.tensor_stats_worklist([(o, n, 0) for _, o, n in running], dev)
            self._rws = ops.tensor_stats_workspace(self._rtab["nitems"], 1, dev)
            nrec += self._rtab["nseg"]
        self._nrec = nrec
        self._out = torch.zeros(max(nrec, 1) * ops.TSTAT_BYTES, dtype=torch.uint8, device=dev)
        self._sync_pending()                                           # (copies into the old ring must land before it goes)
        self._ring = torch.zeros(RING, max(nrec, 1) * ops.TSTAT_BYTES, dtype=torch.uint8).pin_memory()
        self._key = key

    def _buffers(self, st):
        out = []
        for w in self._flat:
            if w == "param":
                b = st.P
            elif w == "grad":
                b = st.G
            else:
                b = getattr(self.optimizer, _MOMENTS[w][1])
                if b is None or b.device != st.P.device:
                    raise L.DykError("TensorStats: the optimizer has no %s yet (it allocates its moments at the first step)" % w)
            out.append(b)
        return out

    # ------------------------------------------------------------------ device side
    def launch(self):
        """Enqueue on the current stream: the two dyk_tensor_stats launches per table, then an asynchronous copy of the records
        into a pinned ring of eight slots with an event each.  No host synchronisation (unless the host runs a whole ring
        ahead of the device).  Call it between backward() and optimizer.step(): the fused step may clear the gradient buffer.
        Data parallel (dyk.ddp.GradAllReduce): call it after reducer.all_reduce(), so that the reduced gradient is read.
        Gradients are reported as stored, NOT multiplied by the optimizer's grad_scale.  Frozen parameters are skipped for
        "grad" and the moments and included for "param"."""
        st = self.model.engine.store
        if st.P is None:
            raise L.DykError("run one forward pass (or model.engine.store.adopt(device)) before TensorStats.launch()")
        self._tables(st)
        nflat = len(self._flat)
        if self._tab is not None:
            ops.tensor_stats(self._buffers(st), self._tab, self._out, self._ws, n=st.total)
        if self._rtab is not None:
            roff = (self._tab["nseg"] * nflat if self._tab is not None else 0) * ops.TSTAT_BYTES
            ops.tensor_stats([st.R], self._rtab, self._out[roff:], self._rws, n=st.rtotal)
        self._poll()
        if len(self._pending) >= RING:           # the host runs a whole ring ahead of the device: wait for the oldest copy
            self._pending[0][1].synchronize()
            self._poll()
        host = self._ring[self._slot % RING]
        self._slot += 1
        host.copy_(self._out, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        meta = dict(flat=self._flat, names=self._names, numels=self._numels, flags=self._flags,
                    nseg=self._tab["nseg"] if self._tab is not None else 0,
                    rnames=self._rnames if self._rtab is not None else None, rnumels=self._rnumels)
        self._pending.append((host, ev, meta))

    def _poll(self):
        landed = None
        while self._pending and self._pending[0][1].query():
            landed = self._pending.pop(0)
        if landed is not None:
            self._last = (landed[0].numpy().tobytes(), landed[2])      # (copied out: the slot is reused)
            self._decoded = None

    def _sync_pending(self):
        if self._pending:
            self._pending[-1][1].synchronize()
            self._poll()

    # ------------------------------------------------------------------ host side
    def read(self, wait=False):
        """{what: {name: Stat(norm, absmax, nonfinite, zeros, numel, sumsq)}} of the newest launch() whose records have
        reached the host, or None; always a complete result.  norm = sqrt(sumsq) over the finite elements; names are those of
        model.named_parameters() ("running": of the buffers); a skipped (frozen) entry is absent.  wait=False never
        synchronises: the answer may be a step or two old.  wait=True waits for the copy behind the last launch()."""
        if wait:
            self._sync_pending()
        elif self._pending:
            self._poll()
        if self._last is None:
            return None
        if self._decoded is None:
            raw, meta = self._last
            flat = meta["flat"]
            res = {w: {} for w in self.what}
            nseg = meta["nseg"]
            if nseg:
                rec = ops.tensor_stats_records(raw, nseg, len(flat))
                for k, w in enumerate(flat):
                    res[w] = self._stats(rec[:, k], meta["names"], meta["numels"], [(f >> k) & 1 for f in meta["flags"]])
            if meta["rnames"] is not None:
                rrec = ops.tensor_stats_records(raw[nseg * len(flat) * ops.TSTAT_BYTES:], len(meta["rnames"]), 1)
                res["running"] = self._stats(rrec[:, 0], meta["rnames"], meta["rnumels"], [0] * len(meta["rnames"]))
            self._decoded = res
        return {w: dict(d) for w, d in self._decoded.items()}

    @staticmethod
    def _stats(col, names, numels, skipped):
        out = {}
        for r, name, numel, skip in zip(col, names, numels, skipped):
            if not skip:
                s = float(r["sumsq"])
                out[name] = Stat(math.sqrt(s), float(r["absmax"]), int(r["nonfinite"]), int(r["zeros"]), int(numel), s)
        return out

    def first_nonfinite(self, which="grad", wait=True):
        """names of the tensors of `which` that hold inf / NaN, in REVERSE store order: the backward pass reaches the deepest
        layer first, so the first name is the likeliest origin.  [] when there is none or nothing has been launched."""
        if which not in self.what:
            raise ValueError("TensorStats: %r is not among what=%r" % (which, self.what))
        r = self.read(wait=wait)
        if r is None:
            return []
        return [n for n, s in reversed(list(r[which].items())) if s.nonfinite > 0]

    def summary(self, k=10):
        """a short text table for logs: the k largest gradient norms (of the first quantity when "grad" is not collected), the
        k largest magnitudes and every non-finite entry"""
        r = self.read(wait=True)
        if r is None:
            return "TensorStats: nothing launched yet"
        lead = "grad" if "grad" in r else self.what[0]
        rows = list(r[lead].items())
        fmt = lambda n, s: "  %-52s norm %-12.5g absmax %-12.5g nonfinite %-8d zeros %d / %d" % (
            n, s.norm, s.absmax, s.nonfinite, s.zeros, s.numel)
        total = math.sqrt(sum(s.sumsq for _, s in rows))
        lines = ["TensorStats %s: %d tensors, norm %.6g" % (lead, len(rows), total), " largest norm:"]
        lines += [fmt(n, s) for n, s in sorted(rows, key=lambda t: -t[1].norm)[:k]]
        lines.append(" largest absmax:")
        lines += [fmt(n, s) for n, s in sorted(rows, key=lambda t: -t[1].absmax)[:k]]
        for w in self.what:
            bad = [(n, s) for n, s in reversed(list(r[w].items())) if s.nonfinite > 0]
            if bad:
                lines.append(" non-finite %s (deepest first):" % w)
                lines += [fmt(n, s) for n, s in bad]
        if not any(s.nonfinite for w in self.what for s in r[w].values()):
            lines.append(" no non-finite entries")
        return "\n".join(lines)
