"""Canonical, process-independent dumps of dry-compiled plans (compile_plan(..., device=cpu, dry=True)) and their digests.

    python tests/golden/make_plan_dumps.py                writes tests/golden/plan_dumps.json (one SHA-256 per case and part)
    python tests/golden/make_plan_dumps.py --full DIR     also writes every whole dump to DIR/<case>.json, for diffing two trees

tests/test_host_plan_dumps.py compiles the same cases and compares the digests: the plan compiler may be restructured freely as
long as every command, every descriptor byte and the arena layout stay what they were when plan_dumps.json was written.

Canonical form.  Every field of every descriptor is written (the ctypes `_fields_`, arrays and padding included), floats as
float.hex().  A non-null pointer becomes [region, byte offset]: the four arenas, the parameter store's P / G / R / NBT, the
compute-weight tensors of the call, the head outputs, plan.io and the tensors kept in plan._keep.  A pointer to another descriptor
becomes that descriptor's canonical form -- or, where it is a command's own descriptor, [list, index] -- never its position in
_keep: descriptors may be created in any order.  A pointer that resolves to nothing raises.
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, os.path.join(ROOT, "double-yolo-kaist_amd"), TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "plan_dumps.json")
PARTS = ("fwd", "bwd", "arenas", "maps")
# the switches a case may set: cleared before every case, so that a digest never depends on the caller's environment
SWITCHES = ("DYK_BNFWD", "DYK_PAIR", "DYK_DEBUG_PLAN", "DYK_KEEP_DZ", "DYK_BNBWD_FUSE", "DYK_WGRAD_PARTIALS", "DYK_WGRAD_GROUP",
            "DYK_DW_PRE", "DYK_WGRAD_RB", "DYK_WGRAD_PS")


def cases():
    """name -> dict(cfg, B, H, W, dtype, training, env, freeze).  cfg: a name of helpers.CFGS, or 'tiny_pool' / 'tiny_shortcut'
    (the two compiling cfgs of test_strided_maxpool_compiles_and_unsupported_sections_fail_loudly)"""
    from helpers import C3, C5, CFGS, INC
    out = {}

    def add(name, cfg, dtype="bf16", training=True, B=2, H=64, W=96, env=None, freeze=None):
        out[name] = dict(cfg=cfg, B=B, H=H, W=W, dtype=dtype, training=training, env=env or {}, freeze=freeze)
    for q, cfg in enumerate(CFGS):
        add("cfg%d_bf16_train" % q, cfg)
        add("cfg%d_bf16_eval" % q, cfg, training=False)
        add("cfg%d_fp32_train" % q, cfg, dtype="fp32")
    add("c3_fp16_eval", C3, dtype="fp16", training=False)
    add("c5_fp16_eval", C5, dtype="fp16", training=False)
    for k, v in (("DYK_BNFWD", "1"), ("DYK_DEBUG_PLAN", "1"), ("DYK_KEEP_DZ", "1"), ("DYK_BNBWD_FUSE", "0"),
                 ("DYK_WGRAD_PARTIALS", "0")):
        add("c3_train_%s=%s" % (k, v), C3, env={k: v})
    add("c5_train_DYK_DW_PRE=1", C5, env={"DYK_DW_PRE": "1"})         # deferred normalise: same command count, other digest
    add("c5_train_DYK_BNBWD_FUSE=0", C5, env={"DYK_BNBWD_FUSE": "0"})
    # the smallest maps: empty parity classes in the strided data gradients, 1x1 / 1x2-pixel deep stages
    add("c3_b1_32x32", C3, B=1, H=32, W=32)
    add("c5_b1_32x32", C5, B=1, H=32, W=32)
    add("inc_b1_32x64", INC, B=1, H=32, W=64)
    add("c3_frozen_backbone", C3, freeze=224)                             # test_frozen_layers_shrink_the_backward_list
    add("tiny_pool", "tiny_pool", B=1, H=64, W=96)
    add("tiny_shortcut", "tiny_shortcut", B=1, H=64, W=64)
    return out


_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_TINY_EXTRA = {"tiny_pool": "",
               "tiny_shortcut": "[convolutional]\nbatch_normalize=1\nfilters=32\nsize=1\nstride=1\npad=1\nactivation=leaky\n\n"
                                "[shortcut]\nfrom=-2\nactivation=linear\n"}


def _model(cfg, tmp_dir):
    from models import YOLO
    torch.manual_seed(0)
    if cfg in _TINY_EXTRA:
        from test_host_plan import TINY_MAXPOOL_CFG
        path = os.path.join(str(tmp_dir), "%s_kaist.cfg" % cfg)
        with open(path, "w") as f:
            f.write(TINY_MAXPOOL_CFG % _TINY_EXTRA[cfg])
        return YOLO(path)
    from build_utils.parse_config import materialize_cfg
    return YOLO(materialize_cfg(cfg))


def compile_case(case, tmp_dir):
    """the plan of one case (the switches of case['env'] are the caller's business), its store and the compute weights it got"""
    from dyk.params import ParamStore
    from dyk.plan import compile_plan
    m = _model(case["cfg"], tmp_dir)
    store = ParamStore(m)
    store.adopt(torch.device("cpu"))
    if case["freeze"] is not None:
        for idx in range(case["freeze"] + 1):
            for p in m.module_list[idx].parameters():
                p.requires_grad_(False)
    captured = []
    alloc = store.alloc_compute

    def alloc_and_note(dtype):
        cw = alloc(dtype)
        captured.append(cw)
        return cw
    store.alloc_compute = alloc_and_note
    try:
        plan = compile_plan(m, store, case["B"], case["H"], case["W"], _DTYPES[case["dtype"]], case["training"],
                            torch.device("cpu"), dry=True)
    finally:
        del store.alloc_compute
    assert len(captured) == 1
    return plan, store, captured[0]


class _Canon:
    def __init__(self, plan, store, cw):
        self.plan = plan
        self.regions = []                      # (name, first byte, bytes), looked up in this order
        for name, a in plan.arenas.items():
            self._tensor("arena." + name, a.tensor)
        for name in ("P", "G", "R", "NBT"):
            self._tensor("store." + name, getattr(store, name))
        for name in ("Wc", "Wt", "Wc_pad", "Wt_pad"):
            self._tensor("cw." + name, cw[name])
        for kind in ("stems", "stems_t"):
            for name in sorted(cw[kind]):
                self._tensor("cw.%s.%s" % (kind, name), cw[kind][name])
        for q, p in enumerate(plan.p_out):
            self._tensor("p_out.%d" % q, p)
        if plan.io is not None:
            self._tensor("io", plan.io)
        self.cmd_of = {}                       # address of a command's descriptor -> [list, index]
        for which in ("fwd", "bwd"):
            for q, (_, d) in enumerate(getattr(plan, which)):
                self.cmd_of.setdefault(ctypes.addressof(d), [which, q])
        self.desc_at, self.kept = {}, []       # other descriptors of plan._keep by address; its tensors / ctypes arrays
        for k in plan._keep:
            if isinstance(k, ctypes.Structure):
                self.desc_at[ctypes.addressof(k)] = k
            elif isinstance(k, torch.Tensor):
                self.kept.append((k.data_ptr(), k.numel() * k.element_size(), k))
            elif isinstance(k, ctypes.Array):
                self.kept.append((ctypes.addressof(k), ctypes.sizeof(k), k))
            else:
                raise TypeError("plan._keep holds a %s" % type(k).__name__)
        self._open = set()

    def _tensor(self, name, t):
        self.regions.append((name, t.data_ptr(), max(t.numel() * t.element_size(), 1)))

    def pointer(self, v, owner, field):
        if not v:
            return None
        if v in self.cmd_of:
            return ["cmd"] + self.cmd_of[v]
        if v in self.desc_at:
            return self.desc(self.desc_at[v])
        for name, lo, n in self.regions:
            if lo <= v < lo + n:
                return [name, v - lo]
        for lo, n, k in self.kept:
            if lo <= v < lo + n:
                # (identified by what it holds, not by where it sits in _keep)
                raw = bytes(k) if isinstance(k, ctypes.Array) else bytes(k.contiguous().view(torch.uint8).numpy())
                return ["keep", n, v - lo, self.kept_bytes(owner, field, raw)]
        raise LookupError("%s.%s = %#x resolves to no region" % (type(owner).__name__, field, v))

    def kept_bytes(self, owner, field, raw):
        """what a table kept in _keep holds: the entries of a grouped weight-gradient launch in canonical form"""
        from dyk import lib as L
        if isinstance(owner, L.DykWgradDesc) and field == "group":
            arr = (L.DykWgradGroupEntry * owner.group_n).from_buffer_copy(raw)
            return [self.desc(e, guard=False) for e in arr]
        raise LookupError("%s.%s points into a kept table of unknown layout" % (type(owner).__name__, field))

    def value(self, v, ctype, owner, field):
        if issubclass(ctype, ctypes.Array):
            return [self.value(v[q], ctype._type_, owner, field) for q in range(ctype._length_)]
        if ctype is ctypes.c_void_p:
            return self.pointer(v, owner, field)
        if ctype in (ctypes.c_float, ctypes.c_double):
            return float(v).hex()
        return int(v)

    def desc(self, d, guard=True):
        key = ctypes.addressof(d)
        if guard:
            if key in self._open:
                raise RecursionError("descriptor cycle through %s" % type(d).__name__)
            self._open.add(key)
        try:
            out = {"_type": type(d).__name__}
            for name, ctype in d._fields_:
                out[name] = self.value(getattr(d, name), ctype, d, name)
            members = self.plan._wg_groups.get(key)
            if members:                           # a grouped weight-gradient launch: its members' own descriptors
                out["_members"] = [self.desc(m) if m is not d else "lead" for m in members]
            return out
        finally:
            if guard:
                self._open.discard(key)

    def commands(self, which):
        return [[int(op), self.desc(d)] for op, d in getattr(self.plan, which)]

    def command_index(self, d, which=None):
        ref = self.cmd_of[ctypes.addressof(d)]
        assert which is None or ref[0] == which
        return ref


def _tref(t):
    return None if t is None else [t.arena, t.off, t.B, t.H, t.W, t.C, t.ld, t.esize]


def _trefs_in(obj, seen):
    """every TRef reachable from a section's record"""
    from dyk.plan import TRef
    if isinstance(obj, TRef):
        yield obj
    elif isinstance(obj, dict):
        if id(obj) in seen:
            return
        seen.add(id(obj))
        for v in obj.values():
            yield from _trefs_in(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _trefs_in(v, seen)


def dump(plan, store, cw):
    """the canonical dump: dict of the four PARTS and the two command counts"""
    c = _Canon(plan, store, cw)
    arenas = {name: dict(size=a.size, blocks=[list(b) for b in a.blocks], pads=sorted([k, v] for k, v in a.pads.items()))
              for name, a in plan.arenas.items()}
    owner = {}                                  # tid -> (first section whose record or output names the tensor, that tensor)
    for i, rec in enumerate(plan.info):
        for t in list(_trefs_in(rec, set())) + ([plan.outs[i]] if plan.outs[i] is not None else []):
            owner.setdefault(t.tid, (i, t))
    grads = []
    for tid, g in plan.grads.items():
        i, t = owner.get(tid, (-1, None))
        grads.append([i, _tref(t), _tref(g)])
    grads.sort(key=lambda e: (e[0], json.dumps(e[1:])))
    maps = dict(
        fwd_lanes=sorted([k, v] for k, v in plan.fwd_lanes.items()), bwd_lanes=sorted([k, v] for k, v in plan.bwd_lanes.items()),
        bwd_marks=[list(m) for m in getattr(plan, "bwd_marks", [])], fwd_layer=list(plan.fwd_layer), bwd_layer=list(plan.bwd_layer),
        late_fused=int(getattr(plan, "late_fused", 0)), bnfwd_counters=list(plan.bnfwd_counters),
        dyn_in=[c.command_index(d) + [key] for d, key in plan.dyn_in],
        dyn_dp=[c.command_index(d, "bwd") + [head] for d, head in plan.dyn_dp],
        stem_fuse=[[c.command_index(ap, "bwd"), c.command_index(wd, "bwd")] for ap, wd in plan.stem_fuse],
        outs=[_tref(t) for t in plan.outs], grads=grads)
    return dict(fwd=c.commands("fwd"), bwd=c.commands("bwd"), arenas=arenas, maps=maps, n_fwd=len(plan.fwd), n_bwd=len(plan.bwd))


def digests(d):
    out = {p: hashlib.sha256(json.dumps(d[p], sort_keys=True, separators=(",", ":")).encode()).hexdigest() for p in PARTS}
    out["n_fwd"], out["n_bwd"] = d["n_fwd"], d["n_bwd"]
    return out


def run_case(case, tmp_dir):
    plan, store, cw = compile_case(case, tmp_dir)
    return dump(plan, store, cw)


@contextlib.contextmanager
def _environment(env):
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", metavar="DIR", help="write every whole dump to DIR/<case>.json")
    args = ap.parse_args()
    if args.full:
        os.makedirs(args.full, exist_ok=True)
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in cases().items():
            with _environment(case["env"]):
                d = run_case(case, tmp)
            rec[name] = digests(d)
            print(name, rec[name]["n_fwd"], rec[name]["n_bwd"], rec[name]["bwd"][:12], flush=True)
            if args.full:
                with open(os.path.join(args.full, name + ".json"), "w") as f:
                    json.dump(d, f, indent=0, sort_keys=True)
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
